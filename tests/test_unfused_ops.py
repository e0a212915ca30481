"""The un-fused operators -- hsk_mf_scores (k_scores, k_bias_scores), hsk_mf_backward (k_backward_dense,
k_bias_backward), hsk_embedding_gather (k_rows_gather), their wrappers in hassaku_amd/hip_ops.py and the autograd
functions of algorithms/sgd_alg.py -- against the float64 numpy restatement tests/ops_restate.py, at every boundary of
their dispatch (the cases and what they reach: tests/ops_cases.py; the claims are checked on the CPU by
tests/test_ops_restate.py).

Exact cases.  Tables hold integers in [-8, 8], biases integers in [-16, 16], the explicit gradient of the logits
integers in [-4, 4]; each case asserts from the restatement's scale that every element's sum of |terms| is below 2^24.
Every product and every partial sum is then an integer that fp32 holds, in any order, atomics included, so scores and
every gradient tensor have to be BIT-EQUAL to the float64 figures rounded to float32: one wrong index, one lost or
doubled atomic, one stale row changes an integer.  Rows nobody indexed are exactly zero, the status word is 0 (or, with
a bad index, the bad-index bit, and the figures are those of the restatement on the clamped indices: row 0).

Rounded cases.  The same shapes on randn * 0.3 tables, randn * 0.1 biases and a randn gradient, every element against
its own scale (derived, not measured; the measured worst cases are printed in the ROW lines, MEASUREMENTS.md):
  scores     |got - f64| <= (NCH * V + 6 + 3) * 2^-24 * (sum_k |U * I| + |Ub| + |Ib| + |gb|): the per-lane fmaf chain is
             NCH * V long, the wave tree has six stages, there are three bias adds
  gradients  |got - f64| <= (n + 1) * 2^-24 * sum |terms|, n the element's term count: valid for any order of the sum
a value below 2^-126 gets the same count of 2^-149 steps, a zero scale demands an exact zero.
"""
import numpy as np
import pytest
import torch

import ops_cases as C
import ops_restate as R
from test_hip_parity import dev

pytestmark = pytest.mark.gpu

MODES = ('exact', 'rounded')
GRAD_NAMES = ('user_emb', 'item_emb', 'item_bias', 'user_bias', 'global_bias')
BAD_INDEX = 1     # HSK_STATUS_BAD_INDEX


@pytest.fixture(scope='module')
def ops():
    from hassaku_amd import hip_ops
    return hip_ops


def _ids(cases):
    return [c['name'] for c in cases]


def _poison(*shape):
    """A freed block of NaNs of the result's size: what torch.empty in the wrapper is likely to be handed, so that an
    element a kernel fails to write shows."""
    t = torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')
    del t


def _poison_grads(case):
    """The same for every gradient buffer of the backward call that follows ([users, D], [items, D], [items], [users],
    [1]): a buffer the operator fails to clear shows in the rows nobody indexed."""
    nu, ni, D = case['n_users'], case['n_items'], case['D']
    blocks = [torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')
              for shape in ([(nu, D), (ni, D)] if D else []) + [(ni,), (nu,), (1,)]]
    del blocks


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _hold(got, ref, scale, tol, mode, what):
    """exact: bit-equal to float64 rounded to float32.  rounded: every element within its own bound.  -> worst
    |err| / bound (0 in exact mode)."""
    got = got.detach().cpu().numpy().reshape(ref.shape)
    assert got.dtype == np.float32, what
    if mode == 'exact':
        assert R.is_exact(scale), (what, 'precondition', float(np.max(scale)))
        bad = np.argwhere(_bits(got) != _bits(ref))
        assert bad.size == 0, (what, len(bad), 'first', bad[0].tolist(), float(got[tuple(bad[0])]),
                               float(ref[tuple(bad[0])]))
        return 0.0
    err = np.abs(got.astype(np.float64) - ref)
    assert np.isfinite(got).all(), what
    over = np.argwhere(err > tol)
    assert over.size == 0, (what, len(over), 'first', over[0].tolist(), float(err[tuple(over[0])]),
                            float(tol[tuple(over[0])]))
    assert (got[scale == 0] == 0).all(), what
    return float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0


def _status(ops, word, want, what):
    assert int(word.item()) == want, what
    if want:
        with pytest.raises(IndexError):
            ops.raise_on_status(word, what)
    else:
        ops.raise_on_status(word, what)


def _run(ops, case, mode):
    """Scores and backward of one case (dim > 0: mf_scores / mf_backward, dim == 0: bias_scores / bias_backward)."""
    T = C.tables(case, mode)
    (s_ref, s_scale, _), G, want_status = C.expected(case, T)
    d = {k: dev(v) for k, v in T.items()}
    u, i = dev(case['u']), dev(case['i'])
    D, B, K = case['D'], case['B'], case['K']
    has = {k: T[k] is not None for k in ('item_bias', 'user_bias', 'global_bias')}
    st_s, st_b = ops.new_status('cuda'), ops.new_status('cuda')
    _poison(B, K)
    if D:
        logits = ops.mf_scores(d['user_emb'], d['item_emb'], d['item_bias'], d['user_bias'], d['global_bias'], u, i, st_s)
        _poison_grads(case)
        grads = ops.mf_backward(d['user_emb'], d['item_emb'], u, i, d['grad'], has['item_bias'], has['user_bias'],
                                has['global_bias'], st_b)
        got = dict(zip(GRAD_NAMES, grads))
    else:
        logits = ops.bias_scores(d['item_bias'], d['user_bias'], d['global_bias'], u, i, st_s)
        _poison_grads(case)
        grads = ops.bias_backward(case['n_users'], case['n_items'], u, i, d['grad'], has['global_bias'], st_b)
        got = dict(zip(GRAD_NAMES[2:], grads))
    assert tuple(logits.shape) == (B, K)
    worst = {'scores': _hold(logits, s_ref, s_scale, R.scores_bound(D, s_scale, s_ref), mode, 'scores')}
    for name, g in got.items():
        if name in has and not has[name]:
            assert g is None, name          # an un-wanted gradient is not formed
            continue
        ref, scale, n = G[name]
        assert tuple(g.shape) == ref.shape, name
        worst[name] = _hold(g, ref, scale, R.grad_bound(scale, n, ref), mode, 'd ' + name)
        assert (g.cpu().numpy()[n == 0] == 0).all(), (name, 'a row nobody indexed is not zero')
    _status(ops, st_s, want_status, 'scores')
    _status(ops, st_b, want_status, 'backward')
    for k, v in T.items():                  # the operands are read only
        if v is not None:
            assert np.array_equal(_bits(d[k].cpu().numpy()), _bits(v)), k
    if mode == 'rounded':
        print(f'ROW unfused {case["name"]}: worst err/bound ' + ' '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    return worst


# ------------------------------------------------------------------------------------------------
# dim > 0
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', C.k_ladder_cases(), ids=_ids(C.k_ladder_cases()))
def test_column_ladder(ops, case, mode):
    """K on both sides of a pass (64), a wave (128), a workgroup (512) and at every remainder against the R buffered
    rows, at D = 64 (R = 4) and D = 1024 (R = 2)."""
    _run(ops, case, mode)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', C.d_ladder_cases(), ids=_ids(C.d_ladder_cases()))
def test_row_shape_ladder(ops, case, mode):
    """Every (V, NCH) pair and both FULL values of hsk_dispatch_dim, with and without a tail chunk."""
    assert R.tile(case['D']) is not None
    _run(ops, case, mode)


def test_row_shape_ladder_reaches_every_tile():
    tiles = {R.tile(D) for D in C.D_LADDER}
    assert {t[:2] for t in tiles} == C.ALL_TILES and {t[2] for t in tiles} == {False, True}


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', C.bias_set_cases(), ids=_ids(C.bias_set_cases()))
def test_bias_sets(ops, case, mode):
    """All eight present / absent combinations: each bias reaches the score once and its own gradient slot, an absent
    one is skipped and its gradient is None."""
    _run(ops, case, mode)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', C.dup_cases(), ids=_ids(C.dup_cases()))
def test_duplicates(ops, case, mode):
    """Heavy duplication: the atomics of a whole row on one item, of a whole batch on one user, the positive among its
    negatives, the tables' last rows."""
    _run(ops, case, mode)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', C.bad_cases(), ids=_ids(C.bad_cases()))
def test_bad_index_reads_row_zero(ops, case, mode):
    """One bad entry (-1, n, 2^40) among valid ones, in u_idx and at the columns 0, 63, 64, 127, 128, K - 1 of i_idx:
    the kernels clamp it to row 0 (hsk_clamp_index) -- scores and gradients are those of the restatement on the clamped
    indices, every other row is untouched, the status word carries the bad-index bit."""
    assert R.is_bad(case['u'], case['n_users']) or R.is_bad(case['i'], case['n_items'])
    _run(ops, case, mode)


@pytest.mark.parametrize('D', C.D_REFUSED)
def test_dimension_past_the_limit_is_refused(ops, D):
    """Just past each alignment's widest row the three operators raise the library's error naming the dimension, touch
    no status word, and the next valid call on the same index and status tensors is exact."""
    case = C.make_case(f'refused-d{D}', R.max_dim(D), 4, 5)
    assert R.tile(D) is None and R.tile(case['D']) is not None
    T = C.tables(case, 'exact')
    rng = np.random.RandomState(D)
    wide = {k: dev(rng.randint(-8, 9, size=(T[k].shape[0], D)).astype(np.float32)) for k in ('user_emb', 'item_emb')}
    u, i, g = dev(case['u']), dev(case['i']), dev(T['grad'])
    status = ops.new_status('cuda')
    msg = f'embedding_dim {D} not supported'
    with pytest.raises(RuntimeError, match=msg):
        ops.mf_scores(wide['user_emb'], wide['item_emb'], None, None, None, u, i, status)
    with pytest.raises(RuntimeError, match=msg):
        ops.mf_backward(wide['user_emb'], wide['item_emb'], u, i, g, True, True, True, status)
    with pytest.raises(RuntimeError, match=msg):
        ops.embedding(wide['item_emb'], i, status)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    (s_ref, s_scale, _), G, _ = C.expected(case, T)
    d = {k: dev(v) for k, v in T.items()}
    logits = ops.mf_scores(d['user_emb'], d['item_emb'], d['item_bias'], d['user_bias'], d['global_bias'], u, i, status)
    _hold(logits, s_ref, s_scale, None, 'exact', 'scores')
    grads = ops.mf_backward(d['user_emb'], d['item_emb'], u, i, g, True, True, True, status)
    for name, got in zip(GRAD_NAMES, grads):
        _hold(got, G[name][0], G[name][1], None, 'exact', 'd ' + name)
    assert torch.equal(ops.embedding(d['item_emb'], i, status), d['item_emb'][i])
    assert int(status.item()) == 0


# ------------------------------------------------------------------------------------------------
# dim == 0
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', C.bias_cases(), ids=_ids(C.bias_cases()))
def test_bias_only_model(ops, case, mode):
    """bias_scores / bias_backward over the K ladder at B = 1, 5, 9 (B * K on both sides of a workgroup's 256 logits),
    with and without the global bias, under duplication and with a bad index."""
    assert case['D'] == 0
    _run(ops, case, mode)


# ------------------------------------------------------------------------------------------------
# the 65 535-row launch limit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_batch_past_the_launch_limit(ops, mode):
    """B = 65 538: mf_scores and bias_scores cut the batch into launches of 65 535 rows (the last three rows are a
    launch of their own); mf_backward and bias_backward refuse it with ValueError before any launch."""
    for D in (C.BATCH_LIMIT['D'], 0):
        case = C.batch_limit_case(D)
        B, K = case['B'], case['K']
        T = C.tables(case, mode)
        s_ref, s_scale, _ = R.scores(T['user_emb'], T['item_emb'], T['item_bias'], T['user_bias'], T['global_bias'],
                                     case['u'], case['i'])
        d = {k: dev(v) for k, v in T.items()}
        u, i = dev(case['u']), dev(case['i'])
        status = ops.new_status('cuda')
        _poison(B, K)
        if D:
            logits = ops.mf_scores(d['user_emb'], d['item_emb'], d['item_bias'], d['user_bias'], d['global_bias'], u, i,
                                   status)
        else:
            logits = ops.bias_scores(d['item_bias'], d['user_bias'], d['global_bias'], u, i, status)
        assert tuple(logits.shape) == (B, K)
        tol = R.scores_bound(D, s_scale, s_ref)
        _hold(logits[65534:], s_ref[65534:], s_scale[65534:], tol[65534:], mode, 'rows 65 534 .. 65 537')
        w = _hold(logits, s_ref, s_scale, tol, mode, 'scores')
        if mode == 'rounded':
            print(f'ROW unfused {case["name"]}: worst err/bound scores {w:.3f}')
        with pytest.raises(ValueError, match='65535'):
            if D:
                ops.mf_backward(d['user_emb'], d['item_emb'], u, i, d['grad'], True, True, True, status)
            else:
                ops.bias_backward(case['n_users'], case['n_items'], u, i, d['grad'], True, status)
        assert int(status.item()) == 0


# ------------------------------------------------------------------------------------------------
# embedding forward (the backward is held by tests/test_key_sort.py)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,n,shape', C.embedding_cases())
def test_embedding_forward_is_the_indexed_table(ops, D, n, shape):
    rng = np.random.RandomState(1000 * D + n)
    table = dev(rng.randn(C.N_ITEMS, D).astype(np.float32))
    idx = rng.randint(0, C.N_ITEMS, size=n if shape is None else shape).astype(np.int64)
    idx.reshape(-1)[-1] = C.N_ITEMS - 1           # the table's last row
    status = ops.new_status('cuda')
    _poison(idx.size, D)
    out = ops.embedding(table, dev(idx), status)
    assert tuple(out.shape) == idx.shape + (D,)
    assert torch.equal(out, table[dev(idx)])
    assert int(status.item()) == 0


@pytest.mark.parametrize('tag', C.BAD_VALUES)
@pytest.mark.parametrize('D', [3, 130, 256, 2044])
def test_embedding_bad_index_reads_row_zero(ops, D, tag):
    rng = np.random.RandomState(D)
    table = dev(rng.randn(C.N_ITEMS, D).astype(np.float32))
    idx = rng.randint(1, C.N_ITEMS, size=9).astype(np.int64)
    idx[4] = {'-1': -1, 'n': C.N_ITEMS, '2^40': 1 << 40}[tag]
    status = ops.new_status('cuda')
    out = ops.embedding(table, dev(idx), status)
    assert torch.equal(out, table[dev(R.clamp(idx, C.N_ITEMS))])
    assert torch.equal(out[4], table[0])
    _status(ops, status, BAD_INDEX, 'embedding')


# ------------------------------------------------------------------------------------------------
# module level: the autograd functions of algorithms/sgd_alg.py
# ------------------------------------------------------------------------------------------------
PARAM_OF = {'user_emb': 'user_embeddings.weight', 'item_emb': 'item_embeddings.weight',
            'item_bias': 'item_bias.weight', 'user_bias': 'user_bias.weight', 'global_bias': 'global_bias'}
MODULE_ITEMS = 600       # a 513-item list without repeats fits


def _model(case, T):
    """SGDMatrixFactorization with the case's bias flags (dim > 0) or SGDBaseline (dim == 0), the case's integer
    tables copied into its parameters."""
    from hassaku_amd.algorithms.sgd_alg import SGDBaseline, SGDMatrixFactorization
    has_ib, has_ub, has_gb = case['bias']
    if case['D']:
        m = SGDMatrixFactorization(case['n_users'], case['n_items'], case['D'], use_user_bias=has_ub,
                                   use_item_bias=has_ib, use_global_bias=has_gb)
    else:
        m = SGDBaseline(case['n_users'], case['n_items'])
    m = m.cuda()
    params = dict(m.named_parameters())
    want = {PARAM_OF[k] for k, v in T.items() if k in PARAM_OF and v is not None}
    assert set(params) == want
    with torch.no_grad():
        for k, name in PARAM_OF.items():
            if T.get(k) is not None:
                params[name].copy_(dev(T[k]).view(params[name].shape))
    return m, params


def _module_cases():
    out = [C.make_case(f'module-{C._bias_tag(bias)}', 30, 5, 129, bias=bias, n_users=C.N_ITEMS) for bias in C.BIAS_SETS]
    return out + [C.make_case('module-baseline', 0, 5, 129, n_users=C.N_ITEMS)]


@pytest.mark.parametrize('case', _module_cases(), ids=_ids(_module_cases()))
def test_module_training_form(case):
    """model(u [B], i [B, K]) then .backward(integer grad): the output and every p.grad bit-equal to the restatement,
    each gradient with its parameter's own shape ([I, 1], [U, 1], [1]) -- as many users as items, so that a bias
    gradient in the other bias's slot has the right shape and the wrong integers."""
    assert case['n_users'] == case['n_items']
    T = C.tables(case, 'exact')
    (s_ref, s_scale, _), G, _ = C.expected(case, T)
    m, params = _model(case, T)
    out = m(dev(case['u']), dev(case['i']))
    _hold(out, s_ref, s_scale, None, 'exact', 'out')
    out.backward(dev(T['grad']))
    for k, name in PARAM_OF.items():
        if name not in params:
            continue
        p = params[name]
        assert p.grad is not None and p.grad.shape == p.shape, name
        ref, scale, _ = G[k]
        _hold(p.grad, ref.reshape(tuple(p.shape)), scale.reshape(tuple(p.shape)), None, 'exact', name + '.grad')
    m.check_indices()


@pytest.mark.parametrize('case', _module_cases(), ids=_ids(_module_cases()))
def test_module_evaluation_form(case):
    """1-D i_idxs -- a permutation of the catalogue, a 513-item sub-list, a list with repeats: every user against the
    list, scores bit-equal and in the order given (SGDMatrixFactorization: _score_all's general path; SGDBaseline:
    through expand)."""
    case = C.make_case(case['name'] + '-eval', case['D'], 5, 1, bias=case['bias'], n_items=MODULE_ITEMS)
    T = C.tables(case, 'exact')
    m, _ = _model(case, T)
    rng = np.random.RandomState(3)
    u = case['u']
    lists = {'permutation': rng.permutation(MODULE_ITEMS), 'sub-list': rng.permutation(MODULE_ITEMS)[:513],
             'repeats': rng.randint(0, 7, size=130)}
    assert len(set(lists['sub-list'])) == 513 and not np.array_equal(lists['permutation'], np.arange(MODULE_ITEMS))
    for what, items in lists.items():
        items = items.astype(np.int64)
        s_ref, s_scale, _ = R.scores(T['user_emb'], T['item_emb'], T['item_bias'], T['user_bias'], T['global_bias'],
                                     u, np.broadcast_to(items, (len(u), len(items))))
        with torch.no_grad():
            out = m(dev(u), dev(items))
        assert tuple(out.shape) == (len(u), len(items)), what
        _hold(out, s_ref, s_scale, None, 'exact', what)
    m.check_indices()


def test_check_and_clear_status(ops):
    """The check behind every SGD and prototype model's check_indices(): silent on a clear word, raises once on a set one
    (IndexError for a bad index, RuntimeError for a sampler that gave up) and leaves it clear; None is no word."""
    ops.check_and_clear_status(None, 'none')
    word = ops.new_status('cuda')
    ops.check_and_clear_status(word, 'clear')
    for bits, err in ((1, IndexError), (2, RuntimeError), (3, IndexError)):
        word.fill_(bits)
        with pytest.raises(err):
            ops.check_and_clear_status(word, 'set')
        assert int(word.item()) == 0
        ops.check_and_clear_status(word, 'cleared')


@pytest.mark.parametrize('D', [30, 0])
def test_module_check_indices_raises_once(D):
    """check_indices() raises after a bad index, the word is clear afterwards, and the next valid call is exact."""
    case = C.make_case(f'module-bad-d{D}', D, 5, 9, bad=('i', 'n', 2, 4))
    T = C.tables(case, 'exact')
    m, _ = _model(case, T)
    with torch.no_grad():
        m(dev(case['u']), dev(case['i']))
    with pytest.raises(IndexError):
        m.check_indices()
    m.check_indices()          # the word was cleared
    good = C.make_case(f'module-good-d{D}', D, 5, 9)
    (s_ref, s_scale, _), _, _ = C.expected(good, T)
    with torch.no_grad():
        out = m(dev(good['u']), dev(good['i']))
    _hold(out, s_ref, s_scale, None, 'exact', 'out')
    m.check_indices()
