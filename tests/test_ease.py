"""EASE: registry, conf and the numpy restatement against the reference's g12 goldens (CPU); the HIP kernels, the
model and the experiment path against the goldens and the restatement (GPU).

Where a bound is not exact equality it is measured, in the test, from two CPU inverses of the same matrix
(numpy.linalg.inv, which is the reference's, and a Cholesky solve): what two correct fp64 eliminations differ by is
what a third may differ by, times a stated factor.  Every such test prints its bound and the measured value first."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import ease_restate as er
import knn_restate as kr
from conftest import REPO, load_golden

EPS = 2.0 ** -53
GOLD_LAMS = (1, 50, 500)
KS = [100, 50, 10, 5]
# name -> (n_users, n_items, n_interactions) of synthetic.generate(..., seed=3); None = the g11 set
INPUTS = {'g11': None, 's1500': (3000, 1500, 150000), 's2100': (5000, 2100, 400000)}
CASES = [('g11', 1), ('g11', 50), ('g11', 500), ('s1500', 1), ('s1500', 100), ('s2100', 20)]


def _tag(lam):
    return str(lam).replace('.', 'p')


def _gold(lam):
    return load_golden(f'g12_ease_lam{_tag(lam)}.npz')


def _gold_B():
    parts = [load_golden(f'g12_ease_lam50_B{h}.npz') for h in (0, 1)]
    assert int(parts[0]['row0']) == 0 and int(parts[1]['row0']) == parts[0]['B'].shape[0]
    return np.concatenate([p['B'] for p in parts])


@functools.lru_cache(maxsize=None)
def _input(name):
    """(train, val, users): the CSRs of the input and the users whose rows are compared."""
    from hassaku_amd.data.csr import UserItemCsr
    if INPUTS[name] is None:
        fx = load_golden('g11_knn_data.npz')
        n_users, n_items, tr, va, users = int(fx['n_users']), int(fx['n_items']), fx['train'], fx['val'], fx['users']
    else:
        from hassaku_amd.data.synthetic import generate
        d = generate(*INPUTS[name], seed=3)
        n_users, n_items, tr, va = d.n_users, d.n_items, d.train, d.val
        users = np.arange(n_users, dtype=np.int64)
    train = UserItemCsr.from_pairs(tr[:, 0], tr[:, 1], n_users, n_items)
    val = UserItemCsr.from_pairs(va[:, 0], va[:, 1], n_users, n_items)
    return train, val, users


@functools.lru_cache(maxsize=None)
def _restated(name, lam):
    """The restatement of one case: G, both CPU inverses, both score sets, the scale |X||B| and the masked scores."""
    train, _, users = _input(name)
    X = kr.dense_binary(train.indptr, train.indices, train.n_rows, train.n_cols)
    G = er.gram(X, lam)
    P_np, P_ch = er.inv_numpy(G), er.inv_cholesky(G)
    B = er.weights(P_np)
    S = er.score_rows(users, train.indptr, train.indices, B)
    S_ch = er.score_rows(users, train.indptr, train.indices, er.weights(P_ch))
    scale = er.score_rows(users, train.indptr, train.indices, B, absolute=True)
    masked = S.copy()
    for q, u in enumerate(users):
        masked[q, train.row(int(u))] = -np.inf
    return dict(G=G, P_np=P_np, P_ch=P_ch, B=B, S=S, S_ch=S_ch, scale=scale, masked=masked)


def _rel(diff, scale):
    """max over the elements with a non-zero scale of |diff| / scale; elements of zero scale must not differ."""
    assert np.all(diff[scale == 0] == 0)
    nz = scale > 0
    return float((np.abs(diff[nz]) / scale[nz]).max()) if nz.any() else 0.


def _metrics_by_name(ids, label_rows):
    return kr.rank_metrics(ids, label_rows, ks=tuple(KS))


# ------------------------------------------------------------------------------------------------------ CPU
def test_registry_resolves_ease():
    from hassaku_amd.algorithms import algorithms_utils as au
    from hassaku_amd.algorithms.base_classes import SparseMatrixBasedRecommenderAlgorithm
    from hassaku_amd.algorithms.linear_algs import EASE
    assert au.AlgorithmsEnum['ease'].value is EASE and au.AlgorithmsEnum.ease.name == 'ease'
    assert au.AlgorithmsEnum['ease'] is au.LinearAlgorithmsEnum.ease
    assert issubclass(EASE, SparseMatrixBasedRecommenderAlgorithm)
    assert au.ALL_ALGORITHM_NAMES == au.ALGORITHM_NAMES + ('ease',)
    assert set(au.ALGORITHM_NAMES) == {m.name for m in au.AlgorithmsEnum} | {'iknn', 'uknn'}
    assert [m.name for m in au.SparseAlgorithmsEnum] == ['uknn', 'iknn']
    assert 'ease' not in {m.name for m in au.AlgorithmsEnum}
    with pytest.raises(KeyError):
        au.AlgorithmsEnum['slim']


def test_cli_lists_ease():
    out = subprocess.run([sys.executable, os.path.join(REPO, 'run_experiment.py'), '--help'], capture_output=True,
                         text=True, cwd=REPO, check=True).stdout
    assert 'ease' in out and 'iknn' in out and 'mf' in out


@pytest.mark.parametrize('bad, msg', [
    ({}, 'needs lam'),
    ({'lam': 0}, 'int\\(lam\\) >= 1'),
    ({'lam': 0.5}, 'int\\(lam\\) >= 1'),
    ({'lam': -3}, 'int\\(lam\\) >= 1'),
    ({'lam': True}, 'must be a number'),
    ({'lam': '50'}, 'must be a number'),
    ({'lam': float('nan')}, 'finite'),
])
def test_conf_validation(tmp_path, bad, msg):
    from hassaku_amd.algorithms.algorithms_utils import AlgorithmsEnum
    from hassaku_amd.conf.conf_parser import parse_conf
    from hassaku_amd.data.data_utils import DatasetsEnum
    conf = dict(bad, data_path=str(tmp_path), model_save_path=str(tmp_path / 'm'))
    with pytest.raises(ValueError, match=msg):
        parse_conf(conf, AlgorithmsEnum['ease'], DatasetsEnum.ml1m)


def test_conf_builds_model_without_sgd_defaults(tmp_path):
    from hassaku_amd.algorithms.algorithms_utils import AlgorithmsEnum
    from hassaku_amd.algorithms.linear_algs import EASE
    from hassaku_amd.conf.conf_parser import parse_conf
    from hassaku_amd.data.data_utils import DatasetsEnum
    conf = parse_conf({'data_path': str(tmp_path), 'model_save_path': str(tmp_path / 'm'), 'lam': 50.7},
                      AlgorithmsEnum.ease, DatasetsEnum.ml1m)
    assert conf['alg'] == 'ease' and 'lr' not in conf and 'n_epochs' not in conf
    m = AlgorithmsEnum.ease.value.build_from_conf(conf, None)
    assert isinstance(m, EASE) and m.lam == 50.7 and m.lam_int == 50 and m.name == 'EASE'
    with pytest.raises(ValueError):
        EASE(0)


def test_restatement_order_is_scipys():
    """score_rows adds as scipy's csr @ dense does: bitwise X @ B, on the reference's own B."""
    import scipy.sparse as sp
    train, _, _ = _input('g11')
    B = _gold_B()
    X = sp.csr_matrix((np.ones(len(train.indices)), train.indices, train.indptr), shape=(train.n_rows, train.n_cols))
    users = np.arange(train.n_rows)
    assert np.array_equal(er.score_rows(users, train.indptr, train.indices, B), np.asarray(X @ B))


def test_restatement_scores_bitwise_given_reference_weights():
    train, _, users = _input('g11')
    assert np.array_equal(er.score_rows(users, train.indptr, train.indices, _gold_B()), _gold(50)['pred'])


@pytest.mark.parametrize('lam', GOLD_LAMS + (50.7,))
def test_restatement_equals_reference(lam):
    """End to end the restatement repeats the reference's five lines with the same LAPACK call; a different LAPACK
    build may round the inverse differently, so pred is held to the reference's by the element-wise bound of the GPU
    test (8 x the numpy-vs-Cholesky distance, in units of |X||B|), top_ids and metrics exactly on separated users."""
    g = _gold(lam)
    assert float(g['lam']) == lam
    r = _restated('g11', lam)
    tol = 8 * _rel(r['S'] - r['S_ch'], r['scale'])
    got = _rel(r['S'] - g['pred'], r['scale'])
    print(f'lam {lam}: restatement vs reference pred {got:.3e}, bound {tol:.3e}')
    assert got <= tol
    train, val, users = _input('g11')
    ok = er.separated(r['masked'], r['scale'])
    assert (~ok).sum() <= 0.01 * len(users)
    vals, ids = kr.masked_topk(r['S'], [train.row(int(u)) for u in users])
    assert np.array_equal(ids[ok], g['top_ids'][ok])
    assert np.all(g['gap'][ok])                      # a separated user's 100th and 101st reference scores differ
    assert np.all(np.abs(vals - g['top_vals'])[ok] <= tol * np.take_along_axis(r['scale'], ids, 1)[ok])
    met = _metrics_by_name(ids, [val.row(int(u)) for u in users])
    names = list(g['metric_names'])
    for name, v in met.items():
        np.testing.assert_allclose(v[ok], g['metrics'][ok, names.index(name)], rtol=1e-6, atol=1e-7, err_msg=name)


def test_truncation_of_lam():
    """lam = 50.7 is the reference's lam = 50: its fixtures are the same numbers, and so is the restatement."""
    a, b = _gold(50), _gold(50.7)
    for key in ('pred', 'top_vals', 'top_ids', 'metrics'):
        assert np.array_equal(a[key], b[key]), key
    train, _, _ = _input('g11')
    X = kr.dense_binary(train.indptr, train.indices, train.n_rows, train.n_cols)
    assert np.array_equal(er.gram(X, 50.7), er.gram(X, 50))


def test_reference_style_model_npz_loads(tmp_path):
    import torch
    from hassaku_amd.algorithms.linear_algs import EASE
    pred = np.arange(12, dtype=np.float64).reshape(3, 4) / 7
    np.savez(os.path.join(tmp_path, 'model.npz'), pred_mtx=pred)
    m = EASE(5, device='cpu')
    m.load_model_from_path(str(tmp_path))
    assert (m.n_users, m.n_items) == (3, 4)
    got = m.predict(torch.tensor([2, 0]), torch.tensor([[3, 1], [0, 2]]))
    assert got.dtype == torch.float64
    assert np.array_equal(got.numpy(), np.array([[pred[2, 3], pred[2, 1]], [pred[0, 0], pred[0, 2]]]))
    rows = m.score_rows(torch.tensor([1]), excl=(torch.tensor([0, 0, 2, 2]), torch.tensor([1, 3], dtype=torch.int32)))
    assert np.array_equal(rows.numpy(), np.array([[pred[1, 0], -np.inf, pred[1, 2], -np.inf]]))
    np.savez(os.path.join(tmp_path, 'model.npz'), alg=np.array('iknn'))
    with pytest.raises(ValueError, match='iknn'):
        EASE(5, device='cpu').load_model_from_path(str(tmp_path))


def test_model_npz_is_validated(tmp_path):
    """A file whose B or train CSR does not fit its own shapes is refused before anything reaches the device."""
    from hassaku_amd.algorithms.linear_algs import EASE
    good = dict(alg=np.array('ease'), lam=np.float64(5), n_users=np.int64(2), n_items=np.int64(3), B=np.zeros((3, 3)),
                train_indptr=np.array([0, 1, 3]), train_indices=np.array([2, 0, 1], dtype=np.int32))
    np.savez(os.path.join(tmp_path, 'model.npz'), **good)
    m = EASE(5, device='cpu')
    m.load_model_from_path(str(tmp_path))
    assert (m.n_users, m.n_items) == (2, 3) and m.B.shape == (3, 3) and m.train[1].dtype.is_floating_point is False
    for bad, msg in ((dict(B=np.zeros((3, 4))), 'B of model.npz'), (dict(B=np.zeros((2, 2))), 'B of model.npz'),
                     (dict(train_indptr=np.array([0, 1, 2, 3])), 'train CSR'),
                     (dict(train_indptr=np.array([0, 1, 2])), 'train CSR'),
                     (dict(train_indices=np.array([2, 0, 3], dtype=np.int32)), 'train CSR')):
        np.savez(os.path.join(tmp_path, 'model.npz'), **dict(good, **bad))
        with pytest.raises(ValueError, match=msg):
            EASE(5, device='cpu').load_model_from_path(str(tmp_path))


# ------------------------------------------------------------------------------------------------------ GPU
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _model_with(train, B, lam=50):
    from hassaku_amd.algorithms.linear_algs import EASE
    m = EASE(lam)
    m.n_users, m.n_items = train.n_rows, train.n_cols
    m.train = (_dev(train.indptr), _dev(train.indices))
    m.B = _dev(B)
    return m


@pytest.mark.gpu
@pytest.mark.parametrize('name, lam', CASES)
def test_gram_exact(name, lam):
    import torch
    from hassaku_amd import hip_ops
    from hassaku_amd.algorithms.knn_algs import _transpose
    train, _, _ = _input(name)
    n = train.n_cols
    G_ref = _restated(name, lam)['G']
    t_ptr, t_idx, _ = _transpose(_dev(train.indptr), _dev(train.indices), None, train.n_rows, n)
    M = hip_ops.knn_pack_i8(t_ptr, t_idx, n, train.n_rows)
    for block in (128, 640, 1 << 20):
        G = torch.full((n, n + 3), np.nan, dtype=torch.float64, device='cuda')     # leading dimension > n
        for r0 in range(0, n, block):
            r1 = min(r0 + block, n)
            C = hip_ops.knn_gram_i8(M, n, r0, r1)
            hip_ops.ease_gram_f64(C, r1 - r0, r0, lam, G)
        got = G.cpu().numpy()
        assert np.array_equal(got[:, :n], G_ref), block
        assert np.isnan(got[:, n:]).all()


@pytest.mark.gpu
@pytest.mark.parametrize('name, lam', CASES)
def test_inverse_residual_and_distance(name, lam):
    from hassaku_amd import hip_ops
    r = _restated(name, lam)
    G, P_np, P_ch = r['G'], r['P_np'], r['P_ch']
    n = G.shape[0]
    P = hip_ops.ease_inverse_f64(_dev(G)).cpu().numpy()
    eye = np.eye(n)
    res_gpu, res_np = np.abs(G @ P - eye).max(), np.abs(G @ P_np - eye).max()
    print(f'{name} lam {lam} n {n}: residual max|G P - I| gpu {res_gpu:.3e} numpy {res_np:.3e} (bound {4 * res_np:.3e})')
    top = np.abs(P_np).max()
    dist = np.abs(P - P_np).max() / top
    spread = np.abs(P_np - P_ch).max() / top
    bound = max(8 * spread, 64 * EPS)
    print(f'{name} lam {lam}: distance max|P_gpu - P_np|/max|P_np| {dist:.3e}, numpy-vs-Cholesky {spread:.3e}, '
          f'bound {bound:.3e}')
    assert res_gpu <= 4 * res_np
    assert dist <= bound
    if name == 'g11':
        ref = er.inv_refined(G)
        scale = np.abs(ref).max()
        e_gpu = float(np.abs(P.astype(np.longdouble) - ref).max() / scale)
        e_np = float(np.abs(P_np.astype(np.longdouble) - ref).max() / scale)
        print(f'{name} lam {lam}: error to the longdouble-refined inverse gpu {e_gpu:.3e} numpy {e_np:.3e}')
        assert e_gpu <= 4 * e_np


@pytest.mark.gpu
def test_inverse_leading_dimension():
    """A matrix inside a wider buffer is inverted in place and the columns beyond n are left alone."""
    import torch
    from hassaku_amd import hip_ops
    G = _restated('g11', 50)['G']
    n = G.shape[0]
    buf = torch.full((n, n + 7), 3.25, dtype=torch.float64, device='cuda')
    buf[:, :n] = _dev(G)
    hip_ops.ease_inverse_f64(buf)
    got = buf.cpu().numpy()
    assert np.array_equal(got[:, :n], hip_ops.ease_inverse_f64(_dev(G)).cpu().numpy())
    assert np.all(got[:, n:] == 3.25)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize('name, lam', [('g11', 50), ('s1500', 1)])
def test_weights_bitwise(name, lam):
    import torch
    from hassaku_amd import hip_ops
    P = _restated(name, lam)['P_np']
    n = P.shape[0]
    assert np.array_equal(hip_ops.ease_weights(_dev(P)).cpu().numpy(), er.weights(P))
    buf = torch.full((n, n + 5), -1.5, dtype=torch.float64, device='cuda')
    buf[:, :n] = _dev(P)
    got = hip_ops.ease_weights(buf).cpu().numpy()
    assert np.array_equal(got[:, :n], er.weights(P)) and np.all(got[:, n:] == -1.5)


@pytest.mark.gpu
@pytest.mark.parametrize('name, lam', [('g11', 50), ('s1500', 100), ('s2100', 20)])
def test_scores_bitwise_given_weights(name, lam):
    """Fed a host-made B the score rows are bitwise X @ B: users without items give zeros, excluded columns -inf, for
    windows that do and do not divide n_items; a bad user id is reported by check_indices."""
    import torch
    from hassaku_amd.data.csr import UserItemCsr
    train, val, users = _input(name)
    B = _gold_B() if name == 'g11' else _restated(name, lam)['B']
    # the same matrix with the items of a few users removed
    keep = ~np.isin(np.repeat(np.arange(train.n_rows), np.diff(train.indptr)), [0, 7, train.n_rows - 1])
    rows = np.repeat(np.arange(train.n_rows), np.diff(train.indptr))[keep]
    holed = UserItemCsr.from_pairs(rows, train.indices[keep], train.n_rows, train.n_cols)
    all_users = np.arange(train.n_rows, dtype=np.int64)
    for csr in (train, holed):
        exp = er.score_rows(all_users, csr.indptr, csr.indices, B)
        m = _model_with(csr, B)
        for w in (7, 64, 100, 1024, 4096):
            m.WINDOW = w
            assert np.array_equal(m.score_rows(_dev(all_users)).cpu().numpy(), exp), w
        if csr is holed:
            assert np.all(exp[[0, 7, -1]] == 0) and not np.signbit(m.score_rows(_dev(all_users[:1])).cpu().numpy()).any()
        ep, ei = val.to_device('cuda')
        masked = exp.copy()
        for u in all_users:
            masked[u, val.row(int(u))] = -np.inf
        for w in (100, 1024):
            m.WINDOW = w
            out = torch.empty((len(all_users), train.n_cols), dtype=torch.float64, device='cuda')
            got = m.score_rows(_dev(all_users), excl=(ep, ei), out=out)
            assert got.data_ptr() == out.data_ptr() and np.array_equal(got.cpu().numpy(), masked), w
        m.check_indices()
    if name == 'g11':
        assert np.array_equal(_model_with(train, B).score_rows(_dev(users)).cpu().numpy(), _gold(50)['pred'])
    m = _model_with(train, B)
    m.score_rows(_dev(np.array([1, train.n_rows, 2], dtype=np.int64)))
    with pytest.raises(IndexError):
        m.check_indices()
    m.score_rows(_dev(np.array([-1], dtype=np.int64)))
    with pytest.raises(IndexError):
        m.check_indices()
    m.check_indices()      # the word was cleared


@pytest.mark.gpu
def test_scores_beyond_one_grid_of_rows():
    """65 535 + 3 user ids in one call (the launcher splits the rows at the grid's 65 535): every row is bitwise the
    row a 5-row call gives for that user.  5 users, one without items, 70 items in three windows of 32 (the last
    partial) and an exclusion CSR."""
    import torch
    from hassaku_amd.data.csr import UserItemCsr
    rng = np.random.RandomState(11)
    ur, uc = np.nonzero(rng.rand(5, 70) < 0.3)
    train = UserItemCsr.from_pairs(ur[ur != 3], uc[ur != 3], 5, 70)
    er_, ec_ = np.nonzero(rng.rand(5, 70) < 0.2)
    ep, ei = UserItemCsr.from_pairs(er_, ec_, 5, 70).to_device('cuda')
    m = _model_with(train, rng.standard_normal((70, 70)))
    m.WINDOW = 32
    ids = torch.arange(65535 + 3, device='cuda') % 5
    few = m.score_rows(torch.arange(5, device='cuda'), excl=(ep, ei))
    assert torch.isinf(few).any() and bool((few[3][~torch.isinf(few[3])] == 0).all())
    many = m.score_rows(ids, excl=(ep, ei))
    assert many.shape == (65535 + 3, 70) and torch.equal(many, few[ids])
    m.check_indices()


@pytest.mark.gpu
@pytest.mark.parametrize('name, lam', CASES + [('g11', 50.7)])
def test_fit_scores_ranking_metrics(name, lam):
    """After fit: |S_gpu - S_ref| <= tol (|X||B_ref|) element by element, tol = 8 x the same quantity between the
    restatement with numpy's inverse and with the Cholesky inverse; top-100 ids and per-user metrics equal the
    reference's on every user whose reference top-101 is separated by 1e-10 x its largest |X||B| entry (at most 1 % of
    the users may fall below that).  On g11 the ids and metrics are the committed golden's."""
    import torch
    from hassaku_amd import hip_ops
    from hassaku_amd.algorithms.linear_algs import EASE
    train, val, users = _input(name)
    r = _restated(name, lam)
    m = EASE(lam)
    m.fit(train)
    u = _dev(users)
    S = m.score_rows(u).cpu().numpy()
    tol = 8 * _rel(r['S'] - r['S_ch'], r['scale'])
    got = _rel(S - r['S'], r['scale'])
    print(f'{name} lam {lam}: scores max |S_gpu - S_ref| / (|X||B|) {got:.3e}, bound {tol:.3e}')
    assert np.all(np.abs(S - r['S']) <= tol * r['scale'])
    assert np.array_equal(m.weights(), m.B.cpu().numpy()) and np.all(np.diag(m.weights()) == 0)
    ok = er.separated(r['masked'], r['scale'])
    print(f'{name} lam {lam}: {int((~ok).sum())} of {len(users)} users below the separation window')
    assert (~ok).sum() <= 0.01 * len(users)
    ep, ei = train.to_device('cuda')
    ids = hip_ops.knn_topk_rows(m.score_rows(u, excl=(ep, ei)), 100)[1]
    lp, li = val.to_device('cuda')
    met = hip_ops.rank_metrics(ids, u, lp, li, KS).cpu().numpy()
    ids = ids.cpu().numpy()
    if name == 'g11':
        g = _gold(lam)
        ref_ids = g['top_ids']
        names = list(g['metric_names'])
        ref_met = {nm: g['metrics'][:, names.index(nm)] for nm in names}
    else:
        _, ref_ids = kr.masked_topk(r['S'], [train.row(int(x)) for x in users])
        ref_met = _metrics_by_name(ref_ids, [val.row(int(x)) for x in users])
    assert np.array_equal(ids[ok], ref_ids[ok])
    for t, kk in enumerate(KS):
        for j, nm in enumerate(('precision', 'recall', 'ndcg')):
            np.testing.assert_allclose(met[ok, t, j], ref_met[f'{nm}@{kk}'][ok], rtol=1e-6, atol=1e-7,
                                       err_msg=f'{nm}@{kk}')
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_fit_refuses_what_does_not_fit():
    from hassaku_amd.algorithms.linear_algs import EASE
    from hassaku_amd.data.csr import UserItemCsr
    n_items = 400_000                      # G alone would take 1.28 TB
    huge = UserItemCsr.from_pairs(np.arange(10), np.arange(10) * 7, 10, n_items)
    with pytest.raises(ValueError, match='needs .* bytes of device memory, .* are free'):
        EASE(10).fit(huge)


@pytest.mark.gpu
def test_save_load_score_rows_stable(tmp_path):
    from hassaku_amd.algorithms.linear_algs import EASE
    train, _, users = _input('g11')
    m = EASE(50)
    m.fit(train)
    u = _dev(np.arange(train.n_rows, dtype=np.int64))
    ep, ei = train.to_device('cuda')
    before, before_x = m.score_rows(u).cpu().numpy(), m.score_rows(u, excl=(ep, ei)).cpu().numpy()
    m.save_model_to_path(str(tmp_path))
    with np.load(os.path.join(tmp_path, 'model.npz')) as f:
        assert str(f['alg']) == 'ease' and float(f['lam']) == 50 and f['B'].shape == (train.n_cols, train.n_cols)
        assert 'pred_mtx' not in f
    m2 = EASE(50)
    m2.load_model_from_path(str(tmp_path))
    assert np.array_equal(m2.score_rows(u).cpu().numpy(), before)
    assert np.array_equal(m2.score_rows(u, excl=(ep, ei)).cpu().numpy(), before_x)
    # the reference's form: a dense pred_mtx
    os.makedirs(tmp_path / 'ref')
    np.savez(os.path.join(tmp_path, 'ref', 'model.npz'), pred_mtx=before)
    m3 = EASE(50)
    m3.load_model_from_path(str(tmp_path / 'ref'))
    assert np.array_equal(m3.score_rows(u).cpu().numpy(), before)
    assert np.array_equal(m3.score_rows(u, excl=(ep, ei)).cpu().numpy(), before_x)
    m3.check_indices()


@pytest.mark.gpu
def test_run_train_val_test(tmp_path):
    """run_experiment's path with -a ease: conf -> slot -> fit -> val metrics -> model.npz -> test metrics through
    load_model_from_path; both equal FullEvaluator fed the restatement's scores.  A user below the separation window
    may rank differently, so each such user widens the bound on a mean by 1 / (size of the smallest group)."""
    import torch
    from hassaku_amd.algorithms.algorithms_utils import AlgorithmsEnum
    from hassaku_amd.data.csr import UserItemCsr
    from hassaku_amd.data.data_utils import DatasetsEnum
    from hassaku_amd.data.synthetic import generate, write_csv_dataset
    from hassaku_amd.eval.eval import FullEvaluator
    from hassaku_amd.experiment_helper import run_train_val_test
    d = generate(250, 180, 6000, seed=7, n_groups=2)
    write_csv_dataset(d, str(tmp_path / 'data' / 'ml100k' / 'processed_dataset'))
    conf = {'data_path': str(tmp_path / 'data'), 'model_save_path': str(tmp_path / 'models'), 'lam': 30.9,
            'eval_batch_size': 64, 'running_settings': {'use_wandb': False, 'batch_verbose': False}}
    best, test, conf = run_train_val_test(AlgorithmsEnum['ease'], DatasetsEnum.ml100k, conf)
    assert os.path.isfile(os.path.join(conf['model_path'], 'model.npz'))
    train = UserItemCsr.from_pairs(d.train[:, 0], d.train[:, 1], d.n_users, d.n_items)
    X = kr.dense_binary(train.indptr, train.indices, d.n_users, d.n_items)
    B = er.fit(X, 30)
    users = np.arange(d.n_users)
    S = er.score_rows(users, train.indptr, train.indices, B)
    scale = er.score_rows(users, train.indptr, train.indices, B, absolute=True)
    groups = torch.as_tensor(np.asarray(d.user_group), dtype=torch.int64)
    smallest = int(np.bincount(np.asarray(d.user_group)).min())
    for split, got in (('val', best), ('test', test)):
        excl_pairs = d.train if split == 'val' else np.concatenate([d.train, d.val])
        excl = UserItemCsr.from_pairs(excl_pairs[:, 0], excl_pairs[:, 1], d.n_users, d.n_items)
        lab_pairs = getattr(d, split)
        labels = kr.dense_binary(*(lambda c: (c.indptr, c.indices))(
            UserItemCsr.from_pairs(lab_pairs[:, 0], lab_pairs[:, 1], d.n_users, d.n_items)), d.n_users, d.n_items)
        masked = S.copy()
        for q in users:
            masked[q, excl.row(int(q))] = -np.inf
        ok = er.separated(masked, scale)
        assert (~ok).sum() <= 0.01 * d.n_users
        ev = FullEvaluator(aggr_by_group=True, n_groups=2, user_to_user_group=groups)
        ev.eval_batch(torch.from_numpy(users), torch.from_numpy(masked), torch.from_numpy(labels))
        ref = ev.get_results()
        assert set(ref) <= set(got) and len(ref) == 36
        for name, v in ref.items():
            assert abs(got[name] - v) <= 1e-6 + (~ok).sum() / smallest, (split, name, got[name], v)
