"""Every way the library issues a large-batch training step, held to the CPU oracle over several steps.

The bit-equality tests of test_hip_parity.py tie the pipelined, side-stream and replayed-graph runs to step_sampled; a
bug shared by both arms passes them.  Here each path is compared with oracle.MfOracleTrainer itself, on skewed batches,
over enough steps that rows carry history (lazy user catch-up, item rows with moments, periodic and closing sweeps):

  recorder   step_sampled one batch at a time, reading (u, i) back after every step.  The sampler is keyed on
             (seed, step), so these are the batches every other path must draw; the oracle replays them.
  single     step_sampled with hint_next (side-stream prefetch)
  pipelined  hint_after_run(n_batches=2) + steps_sampled in three runs, as bench.py issues them, pipeline on
  side       the same calls with the in-launch pipeline switched off
  graph      steps_sampled of >= 64 steps (one replayed graph) plus a few eager tail steps

Each row asserts the partition count P it expects (hsk_part_rule: item table up to 4.5 MB -> 1, 12 -> 2, 24 -> 4,
48 -> 8, halved while N < 8 P) and the pipelined_steps / graph_replays it expects, so a changed rule shows up as a
failed expectation and not as lost coverage.  Tolerances are conftest's: loss sum 1e-6 relative, parameters by
assert_adam_param_close, exp_avg / exp_avg_sq 1e-5 of the tensor's largest."""
import numpy as np
import pytest
import torch

from conftest import ADAM_FRAC, ADAM_MAX_TOL, assert_adam_param_close, csr_from_pairs, max_norm_err
from test_hip_parity import _fused_state, dev

pytestmark = pytest.mark.gpu

SEED = 5
# name: users, items, D, B, N, expected P, steps, loss, optimiser, sampler, lr, wd
SCENARIOS = {
    'headline':     dict(U='ml10m', I=10677, D=512, B=4096, N=100, P=4, steps=8, loss='bpr', opt='adamw', lr=3e-4, wd=4e-5),
    'p2-d256':      dict(U=700, I=8000, D=256, B=2048, N=17, P=2, steps=8, loss='bpr', opt='adamw'),
    'p2-by-nneg':   dict(U=1500, I=10677, D=512, B=3072, N=17, P=2, steps=6, loss='bce', opt='adamw'),   # 4 by size, 2 by N < 32
    'p8-d512':      dict(U=1500, I=16000, D=512, B=4096, N=100, P=8, steps=6, loss='bpr', opt='adamw'),
    'p8-d1024':     dict(U=1500, I=8000, D=1024, B=2048, N=64, P=8, steps=6, loss='bpr', opt='adam'),
    'p2-d1024':     dict(U=1000, I=2000, D=1024, B=2048, N=16, P=2, steps=6, loss='bce', opt='adamw'),
    'p4-d2048':     dict(U=1000, I=2000, D=2048, B=2048, N=33, P=4, steps=6, loss='bpr', opt='adamw'),
    'popular':      dict(U=1500, I=10677, D=512, B=4096, N=100, P=4, steps=6, loss='bpr', opt='adamw', popular=True),
    'ssm-large':    dict(U=700, I=8000, D=256, B=2048, N=17, P=1, steps=6, loss='sampled_softmax', opt='adamw'),
    'ml1m-graph':   dict(U=600, I=3706, D=402, B=128, N=50, P=1, steps=70, loss='bpr', opt='adamw'),
    'ml100k-graph': dict(U=400, I=1682, D=64, B=128, N=1, P=1, steps=70, loss='bpr', opt='adamw'),   # grouped preparation
    'big-graph':    dict(U=900, I=700, D=128, B=2048, N=10, P=1, steps=66, loss='bpr', opt='adamw'),
}
# (scenario, lazy user AdamW, paths); the recorder runs for every (scenario, lazy) too
ROWS = [
    ('headline', True, ('pipelined', 'single')),
    ('p2-d256', True, ('pipelined', 'side')),
    ('p2-d256', False, ('pipelined', 'side')),
    ('p2-by-nneg', False, ('pipelined',)),
    ('p8-d512', True, ('pipelined', 'single')),
    ('p8-d1024', True, ('pipelined',)),
    ('p2-d1024', True, ('pipelined',)),
    ('p4-d2048', False, ('pipelined', 'single')),
    ('popular', True, ('pipelined',)),
    ('ssm-large', True, ('single',)),
    ('ml1m-graph', True, ('graph',)),
    ('ml1m-graph', False, ('graph',)),
    ('ml100k-graph', False, ('graph',)),
    ('big-graph', True, ('graph',)),
]
CASES = [(name, lazy, path) for name, lazy, paths in ROWS for path in ('recorder',) + paths]


@pytest.fixture(scope='module')
def ops():
    from hassaku_amd import hip_ops
    return hip_ops


def _skewed_pairs(rng, n_users, n_items, per_user=12, alpha=1.1):
    """Interactions whose items follow a power law (rank ** -alpha): with rows this short the most popular item is in
    most users' rows, so a batch holds it hundreds of times and the item pass sums that many gradient rows into one item
    row (about 10 000 under the `popular` sampler, whose alias table follows these counts).  User 0 has more than 1024 positives (beyond the sampler's prefetched registers and its LDS row) where the
    catalogue is large enough for that, half the catalogue otherwise."""
    pop = np.arange(1, n_items + 1, dtype=np.float64) ** -alpha
    pop = pop[rng.permutation(n_items)]
    pop /= pop.sum()
    n = np.maximum(1, rng.poisson(per_user, size=n_users))
    users = np.repeat(np.arange(1, n_users, dtype=np.int64), n[1:])
    items = rng.choice(n_items, size=users.size, p=pop)
    heavy = rng.choice(n_items, size=min(1100, n_items // 2), replace=False, p=pop)
    pairs = np.concatenate([np.stack([np.zeros(heavy.size, dtype=np.int64), heavy], axis=1), np.stack([users, items], axis=1)])
    pairs = np.unique(pairs, axis=0)
    return pairs[rng.permutation(len(pairs))]


def _schedule(sc):
    return [(s * sc['B'], sc['B']) for s in range(sc['steps'])]


_DATA = {}


def _data(ops, name, schedule=None):
    """Interactions, initial tables and the interaction order of a scenario (the last one built is kept: the rows of one
    scenario follow each other)."""
    key = (name, None if schedule is None else tuple(schedule))
    if key in _DATA:
        return _DATA[key]
    _DATA.clear()
    sc = dict(SCENARIOS[name])
    sc.setdefault('lr', 1e-3)
    sc.setdefault('wd', 1e-4)
    sc['name'] = name
    sc['schedule'] = _schedule(sc) if schedule is None else list(schedule)
    rng = np.random.RandomState(sum(map(ord, name)))
    if sc['U'] == 'ml10m':
        from hassaku_amd.data import synthetic
        data = synthetic.generate_named('ml10m', seed=0)
        assert data.n_items == sc['I']
        sc['U'] = data.n_users
        pairs = np.ascontiguousarray(data.train[:, :2]).astype(np.int64)
    else:
        pairs = _skewed_pairs(rng, sc['U'], sc['I'])
    U, I, D = sc['U'], sc['I'], sc['D']
    ptr, idx = csr_from_pairs(pairs, U)
    P = {'user_emb': (rng.randn(U, D) * 0.05).astype(np.float32), 'item_emb': (rng.randn(I, D) * 0.05).astype(np.float32),
         'item_bias': (rng.randn(I) * 0.1).astype(np.float32)}
    need = max(s + b for s, b in sc['schedule']) + 2 * sc['B']        # two batches behind the last run may be named
    reps = -(-need // len(pairs))
    order = np.concatenate([np.random.RandomState(6 + r).permutation(len(pairs)) for r in range(reps)])
    alias = None
    if sc.get('popular'):
        alias = ops.build_alias_table(np.bincount(pairs[:, 1], minlength=I).astype(np.float64) ** 0.75 + 1e-3)
    d = dict(sc=sc, pairs=pairs, ptr=ptr, idx=idx, P=P, order=order, alias=alias,
             dev=dict(ptr=dev(ptr), idx=dev(idx), cu=dev(pairs[:, 0], torch.int32), ci=dev(pairs[:, 1], torch.int32),
                      order=torch.from_numpy(order).cuda(),
                      alias=None if alias is None else (dev(alias[0]), dev(alias[1]))))
    _DATA[key] = d
    return d


def _new_state(ops, d, lazy):
    sc, g = d['sc'], d['dev']
    log_adjust = float(np.log(sc['I'] / sc['N'])) if sc['loss'] == 'sampled_softmax' else 0.0
    st, t = _fused_state(ops, d['P'], sc['lr'], sc['wd'], sc['B'], sc['N'] + 1, seed=SEED, csr_indptr=g['ptr'],
                         csr_indices=g['idx'], coo_user=g['cu'], coo_item=g['ci'], lazy_users=lazy, alias=g['alias'],
                         loss=sc['loss'], optimizer=sc['opt'], log_adjust=log_adjust)
    st.st.nnz = g['order'].numel()       # the runs walk `order`, which repeats the interactions
    assert st.batch_columns(sc['B'], sc['N'] + 1) == sc['N'] + sc['P'], ('partitions', sc['name'])
    return st, t


def _snapshot(st, t, d):
    """flush, status, then everything the assertions read"""
    sc = d['sc']
    st.flush()
    st.check_status()
    last = sc['schedule'][-1][1]
    bu, bi = st.last_batch(last, sc['N'] + 1)
    out = dict(loss_sum=st.pop_loss_sum(), last=(bu.cpu().numpy(), bi.cpu().numpy()), steps=st.step_count,
               pipelined=st.pipelined_steps(), replays=st.graph_replays(),
               P={k: v.cpu().numpy().copy() for k, v in t.items()},
               M={k: st.m[k].cpu().numpy().copy() for k in t}, V={k: st.v[k].cpu().numpy().copy() for k in t})
    return out


def _run_recorder(ops, oracle, d, lazy):
    """-> (snapshot, batches [(u, i)], per-step losses); checks every batch against the interactions and the sampler's
    contract (no negative is one of the user's positives)."""
    sc, order = d['sc'], d['dev']['order']
    st, t = _new_state(ops, d, lazy)
    batches, losses = [], []
    for start, nb in sc['schedule']:
        st.step_sampled(order, start, nb, sc['N'])
        u, i = st.last_batch(nb, sc['N'] + 1)
        u, i = u.cpu().numpy(), i.cpu().numpy()
        sel = d['order'][start:start + nb]
        assert np.array_equal(u, d['pairs'][sel, 0]) and np.array_equal(i[:, 0], d['pairs'][sel, 1]), ('positives', start)
        assert oracle.count_bad_negatives(d['ptr'], d['idx'], sc['I'], u, i[:, 1:]) == 0, ('negatives', start)
        batches.append((u, i))
        losses.append(st.last_loss())
    return _snapshot(st, t, d), batches, losses


def _runs_of(schedule, n_runs=3):
    """cut a schedule of equal batches into n_runs consecutive runs: [(first step, number of steps)]"""
    n = len(schedule)
    cuts = [n * k // n_runs for k in range(n_runs + 1)]
    return [(cuts[k], cuts[k + 1] - cuts[k]) for k in range(n_runs) if cuts[k + 1] > cuts[k]]


def _run_path(ops, d, lazy, path):
    sc, order = d['sc'], d['dev']['order']
    B, N, sched = sc['B'], sc['N'], sc['schedule']
    lib = ops._lib.load()
    try:
        lib.hsk_bprmf_set_pipeline(0 if path == 'side' else 1)
        st, t = _new_state(ops, d, lazy)
        if path == 'single':
            for k, (start, nb) in enumerate(sched):
                if k + 1 < len(sched):
                    st.hint_next(order, sched[k + 1][0], sched[k + 1][1], N)
                st.step_sampled(order, start, nb, N)
        elif path in ('pipelined', 'side'):
            for first, m in _runs_of(sched):
                # the two batches behind the run are named, also behind the last one: the closing flush drops them
                st.hint_after_run(order, sched[first][0] + m * B, B, N, n_batches=2)
                st.steps_sampled(order, sched[first][0], m, B, N)
        elif path == 'graph':
            st.steps_sampled(order, sched[0][0], len(sched), B, N)
        else:
            raise ValueError(path)
        return _snapshot(st, t, d)
    finally:
        lib.hsk_bprmf_set_pipeline(1)


_REF = {}


def _reference(ops, oracle, d, lazy):
    """The recorded batches of the scenario replayed through the oracle (kept for the scenario's other rows)."""
    key = (d['sc']['name'], tuple(d['sc']['schedule']))
    if key not in _REF:
        _REF.clear()
        sc = d['sc']
        snap, batches, losses = _run_recorder(ops, oracle, d, lazy)
        log_adjust = float(np.log(sc['I'] / sc['N'])) if sc['loss'] == 'sampled_softmax' else 0.0
        tr = oracle.MfOracleTrainer(d['P']['user_emb'], d['P']['item_emb'], d['P']['item_bias'], lr=sc['lr'], wd=sc['wd'],
                                    loss=sc['loss'], log_adjust=log_adjust, optimizer=sc['opt'])
        ref_losses = [tr.step(u, i)[0] for u, i in batches]
        _REF[key] = dict(tr=tr, losses=ref_losses, batches=batches, recorder=(lazy, snap, losses))
    return _REF[key]


def _hold_to_oracle(what, got, ref, expect_pipelined, expect_replays, step_losses=None):
    """The assertions of this file.  Every figure is printed before anything is asserted (pytest -s shows the table)."""
    tr = ref['tr']
    loss_ref = float(np.sum(ref['losses']))
    loss_rel = abs(got['loss_sum'] - loss_ref) / abs(loss_ref)
    fig = {}
    for k in got['P']:
        scale = np.abs(tr.P[k]).max()
        err = np.abs(got['P'][k].astype(np.float64) - tr.P[k]).reshape(-1) / (scale if scale > 0 else 1.0)
        fig[k] = (float(err.max()), float((err > 1e-5).mean()), max_norm_err(got['M'][k], tr.M[k]), max_norm_err(got['V'][k], tr.V[k]))
        if err.max() >= ADAM_MAX_TOL or (err > 1e-5).mean() > ADAM_FRAC:
            # Adam's division: a parameter element may be off where exp_avg_sq is tiny although the moments agree
            worst = np.argsort(err)[-5:]
            v = tr.V[k].reshape(-1)
            print(f'  {what} {k}: {int((err > 1e-5).sum())} elements beyond 1e-5; worst five: err {err[worst]}, oracle exp_avg_sq '
                  f'{v[worst]} (tensor max {v.max():.3e})')
    print(f'ROW {what}: steps {got["steps"]} pipelined {got["pipelined"]} replays {got["replays"]} loss_rel {loss_rel:.2e} '
          + ' '.join(f'{k}: p {a:.2e} frac {b:.1e} m {c:.2e} v {e:.2e}' for k, (a, b, c, e) in fig.items()), flush=True)
    assert got['steps'] == len(ref['batches']), what
    assert got['pipelined'] == expect_pipelined, (what, 'pipelined_steps', got['pipelined'])
    assert got['replays'] == expect_replays, (what, 'graph_replays', got['replays'])
    if step_losses is not None:
        for s, (a, b) in enumerate(zip(step_losses, ref['losses'])):
            assert abs(a - b) <= 1e-6 * abs(b), (what, 'loss of step', s, a, b)
    assert loss_rel <= 1e-6, (what, 'loss sum', got['loss_sum'], loss_ref)
    assert np.array_equal(got['last'][0], ref['batches'][-1][0]) and np.array_equal(got['last'][1], ref['batches'][-1][1]), \
        (what, 'last batch')
    for k in got['P']:
        assert max_norm_err(got['M'][k], tr.M[k]) < 1e-5, (what, 'exp_avg', k, fig[k][2])
        assert max_norm_err(got['V'][k], tr.V[k]) < 1e-5, (what, 'exp_avg_sq', k, fig[k][3])
    for k in got['P']:
        assert_adam_param_close(got['P'][k], tr.P[k], (what, k))


@pytest.mark.parametrize('name,lazy,path', CASES, ids=[f'{n}-{"lazy" if lz else "dense"}-{p}' for n, lz, p in CASES])
def test_step_path_vs_oracle(ops, oracle, name, lazy, path):
    """One row of the table above: the path's tables, moments, loss sum and last batch against the oracle's replay of the
    recorded batches.  Rows the library would refuse were not met: every (P, D) of the table runs as stated."""
    d = _data(ops, name)
    sc = d['sc']
    ref = _reference(ops, oracle, d, lazy)
    what = f'{name}-{"lazy" if lazy else "dense"}-{path}'
    if path == 'recorder':
        rl, snap, losses = ref['recorder']
        if rl != lazy:
            snap, batches, losses = _run_recorder(ops, oracle, d, lazy)
            for (u0, i0), (u1, i1) in zip(batches, ref['batches']):
                assert np.array_equal(u0, u1) and np.array_equal(i0, i1), 'the draw depends on (seed, step) only'
        _hold_to_oracle(what, snap, ref, 0, 0, step_losses=losses)
        return
    got = _run_path(ops, d, lazy, path)
    n = sc['steps']
    _hold_to_oracle(what, got, ref, n if path == 'pipelined' else 0, n // 64 if path == 'graph' else 0)


# ---------------------------------------------------------------------------------------------------
# a replayed run behind a pipelined run that left prepared batches in the pipeline's slots
# ---------------------------------------------------------------------------------------------------
def _stale_sequence(ops, d, hinted, second_batch, pipeline_off):
    sc, order = d['sc'], d['dev']['order']
    B, N = sc['B'], sc['N']
    lib = ops._lib.load()
    try:
        lib.hsk_bprmf_set_pipeline(1)
        st, t = _new_state(ops, d, False)
        if hinted:
            st.hint_after_run(order, 5 * B, B, N, n_batches=2)
        st.steps_sampled(order, 0, 5, B, N)          # pipelined; hinted: two prepared batches stay behind, owner maps claimed
        assert st.pipelined_steps() == 5
        if pipeline_off:
            lib.hsk_bprmf_set_pipeline(0)
        st.steps_sampled(order, 5 * B, 64, second_batch, N)      # not pipelined, 64 steps: one replayed graph
        assert st.graph_replays() == 1 and st.pipelined_steps() == 5
        return _snapshot(st, t, d)
    finally:
        lib.hsk_bprmf_set_pipeline(1)


@pytest.mark.parametrize('trigger', ['pipeline-off', 'smaller-batch'])
def test_graph_run_after_a_pipelined_run_with_a_tail_hint(ops, oracle, trigger):
    """A pipelined run whose tail hint was honoured leaves two sampled batches in the pipeline's slots, their users
    claimed in the owner maps of the buffer sets.  A following run that is not pipelined but long enough for a replayed
    graph (the pipeline switched off, or a batch below 2048) reuses those sets: it must drop the stale batches first,
    as every other path does.  Equal, bit for bit, to the same steps with no hint; and equal to the oracle.  (Both
    variants failed -- every table, loss sums 1.4e-4 / 2.9e-4 apart -- until hsk_bprmf_train_steps reset the pipeline
    on its branches that are not pipelined: MEASUREMENTS.md.)"""
    sc0 = SCENARIOS['p2-d256']
    B = sc0['B']
    B2 = B if trigger == 'pipeline-off' else 1024
    schedule = [(s * B, B) for s in range(5)] + [(5 * B + s * B2, B2) for s in range(64)]
    d = _data(ops, 'p2-d256', schedule)
    ref = _reference(ops, oracle, d, False)
    a = _stale_sequence(ops, d, True, B2, trigger == 'pipeline-off')
    b = _stale_sequence(ops, d, False, B2, trigger == 'pipeline-off')
    diff = [k for k in a['P'] if not np.array_equal(a['P'][k], b['P'][k])]
    diff += ['m_' + k for k in a['M'] if not np.array_equal(a['M'][k], b['M'][k])]
    diff += ['v_' + k for k in a['V'] if not np.array_equal(a['V'][k], b['V'][k])]
    print(f'ROW stale-{trigger}: hinted vs unhinted differ in {diff}, loss sums {a["loss_sum"]!r} {b["loss_sum"]!r}', flush=True)
    _hold_to_oracle(f'stale-{trigger}-unhinted', b, ref, 5, 1)
    assert not diff, diff
    assert a['loss_sum'] == b['loss_sum']
    assert np.array_equal(a['last'][0], b['last'][0]) and np.array_equal(a['last'][1], b['last'][1])
    _hold_to_oracle(f'stale-{trigger}-hinted', a, ref, 5, 1)
