"""P3alpha: registry, conf, persistence and the numpy restatement against the reference's g13 goldens (CPU); the HIP
kernels, the model and the experiment path against the goldens and the restatement (GPU).

Every term of a P3alpha score is positive, so the bounds are derived, not measured: an entry (u, j) is a sum of
T[u, j] = (X X^T X)[u, j] positive three-factor products, each side is off by at most about (T + 6) 2^-53 relative, the
power multiplies that by alpha and the two pows add 17 ulp (p3alpha_restate.rtol).  An entry is 0.0 exactly where
T = 0.  Every test that uses a bound prints the bound and the measured value first.

Inputs: g11 (300 x 200: 2 x 2 output tiles with a ragged edge, five k blocks, the last one partial), s1500
(generate(3000, 1500, 150000, seed=3): 12 x 12 tiles, 47 k blocks) and islands (130 x 150, two disjoint communities,
users 0, 7, 129 and items 3, 149 empty, 51.5 % of the entries with T = 0)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import knn_restate as kr
import p3alpha_restate as pr
from conftest import REPO, load_golden

ULP = 2.0 ** -52
GOLD_ALPHAS = (1.9, 1.0, 0.5)
KS = [100, 50, 10, 5]
FIT_CASES = [('g11', 1.9), ('g11', 1.0), ('g11', 0.5), ('s1500', 1.9), ('islands', 1.9)]


def _gold(alpha):
    return load_golden(f"g13_p3alpha_a{str(alpha).replace('.', 'p')}.npz")


@functools.lru_cache(maxsize=None)
def _input(name):
    """(train, val, users): the CSRs of the input and the users whose rows are compared."""
    from hassaku_amd.data.csr import UserItemCsr
    if name == 'islands':
        rng = np.random.RandomState(1)
        X = rng.rand(130, 150) < 0.15
        X[:60, 70:] = False
        X[60:, :70] = False
        X[[0, 7, 129]] = False
        X[:, [3, 149]] = False
        rows, cols = np.nonzero(X)
        train = UserItemCsr.from_pairs(rows, cols, 130, 150)
        return train, None, np.arange(130, dtype=np.int64)
    if name == 'g11':
        fx = load_golden('g11_knn_data.npz')
        n_users, n_items, tr, va, users = int(fx['n_users']), int(fx['n_items']), fx['train'], fx['val'], fx['users']
    else:
        from hassaku_amd.data.synthetic import generate
        d = generate(3000, 1500, 150000, seed=3)
        n_users, n_items, tr, va = d.n_users, d.n_items, d.train, d.val
        users = np.arange(n_users, dtype=np.int64)
    train = UserItemCsr.from_pairs(tr[:, 0], tr[:, 1], n_users, n_items)
    val = UserItemCsr.from_pairs(va[:, 0], va[:, 1], n_users, n_items)
    return train, val, users


@functools.lru_cache(maxsize=None)
def _model(name):
    """What does not depend on alpha: X, the reciprocal degrees, the counts, S, W and the path counts T."""
    train, _, users = _input(name)
    X = kr.dense_binary(train.indptr, train.indices, train.n_rows, train.n_cols)
    w_u, w_i = pr.inv_degrees(X.sum(1)), pr.inv_degrees(X.sum(0))
    S = pr.gram(X, w_u)
    T = pr.paths(X)
    return dict(X=X, w_u=w_u, w_i=w_i, C=pr.counts(X), S=S, W=pr.weights(S, w_i), T=T[users], t_max=int(T.max()))


@functools.lru_cache(maxsize=None)
def _restated(name, alpha):
    train, _, users = _input(name)
    m = _model(name)
    S = pr.score_rows(users, train.indptr, train.indices, m['W'], m['w_u'], alpha)
    masked = S.copy()
    for q, u in enumerate(users):
        masked[q, train.row(int(u))] = -np.inf
    return dict(S=S, masked=masked)


def _rel(got, ref):
    """max |got - ref| / ref over the entries with ref > 0; the zero patterns must be equal (and the zeros +0.0)."""
    assert np.array_equal(got == 0, ref == 0)
    assert not np.signbit(got[got == 0]).any()
    nz = ref > 0
    return float((np.abs(got[nz] - ref[nz]) / ref[nz]).max()) if nz.any() else 0.


# ------------------------------------------------------------------------------------------------------ CPU
def test_registry_resolves_p3alpha():
    from hassaku_amd.algorithms import algorithms_utils as au
    from hassaku_amd.algorithms.base_classes import SparseMatrixBasedRecommenderAlgorithm
    from hassaku_amd.algorithms.graph_algs import P3alpha
    assert au.AlgorithmsEnum['p3alpha'].value is P3alpha and au.AlgorithmsEnum.p3alpha.name == 'p3alpha'
    assert au.AlgorithmsEnum['p3alpha'] is au.GraphAlgorithmsEnum.p3alpha
    assert issubclass(P3alpha, SparseMatrixBasedRecommenderAlgorithm)
    assert au.REGISTERED_ALGORITHM_NAMES == au.ALL_ALGORITHM_NAMES + ('p3alpha',)
    # the four pinned objects are what they were
    assert [m.name for m in au.AlgorithmsEnum] == ['mf', 'sgdbias', 'uprotomf', 'iprotomf', 'uiprotomf', 'acf']
    assert [m.name for m in au.SparseAlgorithmsEnum] == ['uknn', 'iknn']
    assert au.ALGORITHM_NAMES == ('mf', 'sgdbias', 'uprotomf', 'iprotomf', 'uiprotomf', 'acf', 'uknn', 'iknn')
    assert au.ALL_ALGORITHM_NAMES == au.ALGORITHM_NAMES + ('ease',)
    with pytest.raises(KeyError):
        au.AlgorithmsEnum['rp3beta']


def test_cli_lists_p3alpha():
    out = subprocess.run([sys.executable, os.path.join(REPO, 'run_experiment.py'), '--help'], capture_output=True,
                         text=True, cwd=REPO, check=True).stdout
    assert 'p3alpha' in out and 'ease' in out and 'iknn' in out and 'mf' in out


@pytest.mark.parametrize('bad, msg', [
    ({}, 'needs alpha'),
    ({'alpha': 0}, '> 0'),
    ({'alpha': -1.5}, '> 0'),
    ({'alpha': True}, 'must be a number'),
    ({'alpha': '1.9'}, 'must be a number'),
    ({'alpha': float('nan')}, 'finite'),
    ({'alpha': float('inf')}, 'finite'),
])
def test_conf_validation(tmp_path, bad, msg):
    from hassaku_amd.algorithms.algorithms_utils import AlgorithmsEnum
    from hassaku_amd.conf.conf_parser import parse_conf
    from hassaku_amd.data.data_utils import DatasetsEnum
    conf = dict(bad, data_path=str(tmp_path), model_save_path=str(tmp_path / 'm'))
    with pytest.raises(ValueError, match=msg):
        parse_conf(conf, AlgorithmsEnum['p3alpha'], DatasetsEnum.ml1m)


def test_conf_builds_model_without_sgd_defaults(tmp_path):
    from hassaku_amd.algorithms.algorithms_utils import AlgorithmsEnum
    from hassaku_amd.algorithms.graph_algs import P3alpha
    from hassaku_amd.conf.conf_parser import parse_conf
    from hassaku_amd.data.data_utils import DatasetsEnum
    conf = parse_conf({'data_path': str(tmp_path), 'model_save_path': str(tmp_path / 'm'), 'alpha': 0.5},
                      AlgorithmsEnum.p3alpha, DatasetsEnum.ml1m)
    assert conf['alg'] == 'p3alpha' and 'lr' not in conf and 'n_epochs' not in conf
    m = AlgorithmsEnum.p3alpha.value.build_from_conf(conf, None)
    assert isinstance(m, P3alpha) and m.alpha == 0.5 and m.name == 'P3alpha'
    assert P3alpha().alpha == 1.9
    for bad in (0, -2, True, '1', float('nan'), float('inf'), None):
        with pytest.raises(ValueError):
            P3alpha(bad)


def test_restatement_single_common_user_is_its_weight():
    """The restated Gram adds from 0.0: an entry with one common user is that user's weight bitwise, one with none 0."""
    m = _model('islands')
    assert np.all(m['S'][m['C'] == 0] == 0) and np.array_equal(m['S'], m['S'].T)
    ii, jj = np.nonzero(m['C'] == 1)
    common = np.argmax(m['X'][:, ii] * m['X'][:, jj], axis=0)
    assert len(ii) > 100 and np.array_equal(m['S'][ii, jj], m['w_u'][common])


@pytest.mark.parametrize('alpha', GOLD_ALPHAS)
def test_restatement_equals_reference(alpha):
    """The restatement against the reference's own pred_mtx rows: scores within rtol(alpha, T_max), the zero pattern
    that of T, top-100 ids and per-user metrics equal on separated users (at most 1 % may be unseparated)."""
    g = _gold(alpha)
    assert float(g['alpha']) == alpha
    train, val, users = _input('g11')
    m, r = _model('g11'), _restated('g11', alpha)
    assert np.array_equal(r['S'] == 0, m['T'] == 0) and np.array_equal(g['pred'] == 0, m['T'] == 0)
    bound = pr.rtol(alpha, m['t_max'])
    got = _rel(r['S'], g['pred'])
    print(f'alpha {alpha}: restatement vs reference pred {got:.3e}, bound {bound:.3e} (T_max {m["t_max"]})')
    assert got <= bound
    ok = pr.separated(r['masked'])
    print(f'alpha {alpha}: {int((~ok).sum())} of {len(users)} users unseparated')
    assert (~ok).sum() <= 0.01 * len(users)
    vals, ids = kr.masked_topk(r['S'], [train.row(int(u)) for u in users])
    assert np.array_equal(ids[ok], g['top_ids'][ok])
    assert np.all(g['gap'][ok])
    assert np.all(np.abs(vals - g['top_vals'])[ok] <= bound * g['top_vals'][ok])
    met = kr.rank_metrics(ids, [val.row(int(u)) for u in users], ks=tuple(KS))
    names = list(g['metric_names'])
    for name, v in met.items():
        np.testing.assert_allclose(v[ok], g['metrics'][ok, names.index(name)], rtol=1e-6, atol=1e-7, err_msg=name)


@pytest.mark.parametrize('name', ['s1500', 'islands'])
def test_restatement_pattern_on_other_inputs(name):
    """Zero pattern of the restated scores = that of T on the inputs without a golden; s1500 leaves (almost) every user
    separated, islands has the empty users and items it is there for."""
    m, r = _model(name), _restated(name, 1.9)
    assert np.array_equal(r['S'] == 0, m['T'] == 0) and np.isfinite(r['S']).all()
    if name == 's1500':
        assert (~pr.separated(r['masked'])).sum() <= 0.01 * len(r['S'])
    else:
        assert np.all(m['X'][[0, 7, 129]] == 0) and np.all(m['X'][:, [3, 149]] == 0)
        assert np.all(m['X'][:60, 70:] == 0) and np.all(m['X'][60:, :70] == 0)
        assert abs((m['T'] == 0).mean() - 0.515) < 1e-3


def test_reference_style_model_npz_loads(tmp_path):
    import torch
    from hassaku_amd.algorithms.graph_algs import P3alpha
    pred = np.arange(12, dtype=np.float64).reshape(3, 4) / 7
    np.savez(os.path.join(tmp_path, 'model.npz'), pred_mtx=pred)
    m = P3alpha(device='cpu')
    m.load_model_from_path(str(tmp_path))
    assert (m.n_users, m.n_items) == (3, 4)
    got = m.predict(torch.tensor([2, 0]), torch.tensor([[3, 1], [0, 2]]))
    assert got.dtype == torch.float64
    assert np.array_equal(got.numpy(), np.array([[pred[2, 3], pred[2, 1]], [pred[0, 0], pred[0, 2]]]))
    rows = m.score_rows(torch.tensor([1]), excl=(torch.tensor([0, 0, 2, 2]), torch.tensor([1, 3], dtype=torch.int32)))
    assert np.array_equal(rows.numpy(), np.array([[pred[1, 0], -np.inf, pred[1, 2], -np.inf]]))
    for bad in (pred[0], pred.astype(np.int64), pred[None]):
        np.savez(os.path.join(tmp_path, 'model.npz'), pred_mtx=bad)
        with pytest.raises(ValueError, match='dense 2-D float'):
            P3alpha(device='cpu').load_model_from_path(str(tmp_path))
    np.savez(os.path.join(tmp_path, 'model.npz'), alg=np.array('ease'))
    with pytest.raises(ValueError, match='ease'):
        P3alpha(device='cpu').load_model_from_path(str(tmp_path))


def test_reference_written_sparse_pred_mtx_is_refused(tmp_path):
    """The reference hands np.savez its scipy sparse pred_mtx: numpy pickles it as an object array, which the
    reference's own np.load cannot read back.  It is refused with a message that says so, and never unpickled."""
    import scipy.sparse as sp
    from hassaku_amd.algorithms.graph_algs import P3alpha
    np.savez(os.path.join(tmp_path, 'model.npz'), pred_mtx=sp.csr_matrix(np.eye(3)))
    with np.load(os.path.join(tmp_path, 'model.npz'), allow_pickle=False) as f:
        with pytest.raises(ValueError):
            f['pred_mtx']
    m = P3alpha(device='cpu')
    with pytest.raises(ValueError, match='object array .* cannot read back'):
        m.load_model_from_path(str(tmp_path))
    assert m.pred_mtx is None and m.W is None


def test_model_npz_is_validated(tmp_path):
    """A file whose W or train CSR does not fit its own shapes is refused before anything reaches the device."""
    from hassaku_amd.algorithms.graph_algs import P3alpha
    good = dict(alg=np.array('p3alpha'), alpha=np.float64(0.75), n_users=np.int64(2), n_items=np.int64(3),
                W=np.zeros((3, 3)), train_indptr=np.array([0, 0, 2]), train_indices=np.array([0, 1], dtype=np.int32))
    np.savez(os.path.join(tmp_path, 'model.npz'), **good)
    m = P3alpha(device='cpu')
    m.load_model_from_path(str(tmp_path))
    assert (m.n_users, m.n_items, m.alpha) == (2, 3, 0.75) and m.W.shape == (3, 3)
    assert m.train[1].dtype.is_floating_point is False and np.array_equal(m.inv_deg_u.numpy(), [0., 0.5])
    for bad, msg in ((dict(W=np.zeros((3, 4))), 'W of model.npz'), (dict(W=np.zeros((2, 2))), 'W of model.npz'),
                     (dict(train_indptr=np.array([0, 1, 2, 2])), 'train CSR'),
                     (dict(train_indptr=np.array([0, 1, 1])), 'train CSR'),
                     (dict(train_indices=np.array([0, 3], dtype=np.int32)), 'train CSR'),
                     (dict(alpha=np.float64(0)), '> 0'), (dict(alpha=np.float64('nan')), 'finite')):
        np.savez(os.path.join(tmp_path, 'model.npz'), **dict(good, **bad))
        with pytest.raises(ValueError, match=msg):
            P3alpha(device='cpu').load_model_from_path(str(tmp_path))


# ------------------------------------------------------------------------------------------------------ GPU
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _model_with(train, W, w_u, alpha):
    from hassaku_amd.algorithms.graph_algs import P3alpha
    m = P3alpha(alpha)
    m.n_users, m.n_items = train.n_rows, train.n_cols
    m.train = (_dev(train.indptr), _dev(train.indices))
    m.W, m.inv_deg_u = _dev(W), _dev(w_u)
    return m


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['g11', 's1500', 'islands'])
def test_gram_weighted(name):
    """hsk_p3_gram_f64 by row blocks of 128, 640 and whole, into a buffer with ld = n + 3: both sides add exactly
    representable terms (w_u or 0), so |got - ref| <= 2^-52 c S with c the integer co-occurrence count; c = 0 gives
    0.0, c = 1 the single w_u bitwise; the matrix is bitwise symmetric; the columns beyond n stay NaN.  Then random
    positive col_weight and a row_scale: the same bound plus one ulp for the scale."""
    import torch
    from hassaku_amd import hip_ops
    from hassaku_amd.algorithms.knn_algs import _transpose
    train, _, _ = _input(name)
    n, n_users = train.n_cols, train.n_rows
    m = _model(name)
    C, S_ref = m['C'], m['S']
    t_ptr, t_idx, _ = _transpose(_dev(train.indptr), _dev(train.indices), None, n_users, n)
    M = hip_ops.knn_pack_i8(t_ptr, t_idx, n, n_users)
    k_pad = M.shape[1]
    w_pad = np.zeros(k_pad)
    w_pad[:n_users] = m['w_u']
    w_dev = hip_ops.p3_inv_degrees(_dev(train.indptr), k_pad)
    assert np.array_equal(w_dev.cpu().numpy(), w_pad)
    assert np.array_equal(hip_ops.p3_inv_degrees(t_ptr).cpu().numpy(), m['w_i'])
    for block in (128, 640, 1 << 20):
        G = torch.full((n, n + 3), np.nan, dtype=torch.float64, device='cuda')
        for r0 in range(0, n, block):
            hip_ops.p3_gram_f64(M, n, w_dev, r0, min(r0 + block, n), G)
        got = G.cpu().numpy()
        assert np.isnan(got[:, n:]).all(), block
        got = got[:, :n]
        assert np.isfinite(got).all()
        nz = C > 0
        worst = float((np.abs(got - S_ref)[nz] / (C * S_ref)[nz]).max() / ULP)
        print(f'{name} block {block}: max |S_gpu - S_ref| / (c S) = {worst:.3f} x 2^-52 (bound 1)')
        assert np.all(np.abs(got - S_ref) <= ULP * C * S_ref)
        assert np.all(got[C == 0] == 0) and not np.signbit(got[C == 0]).any()
        assert np.array_equal(got[C == 1], S_ref[C == 1])
        assert np.array_equal(got, got.T)
    rng = np.random.RandomState(7)
    cw = np.zeros(k_pad)
    cw[:n_users] = rng.rand(n_users) + 0.1
    rs = rng.rand(n) + 0.1
    ref = pr.weights(pr.gram(m['X'], cw[:n_users]), rs)
    G = torch.full((n, n + 3), np.nan, dtype=torch.float64, device='cuda')
    for r0 in range(0, n, 640):
        hip_ops.p3_gram_f64(M, n, _dev(cw), r0, min(r0 + 640, n), G, row_scale=_dev(rs))
    got = G.cpu().numpy()
    assert np.isnan(got[:, n:]).all()
    got = got[:, :n]
    nz = C > 0
    worst = float((np.abs(got - ref)[nz] / ((C + 1) * ref)[nz]).max() / ULP)
    print(f'{name} weighted, scaled: max |got - ref| / ((c + 1) ref) = {worst:.3f} x 2^-52 (bound 1)')
    assert np.all(np.abs(got - ref) <= ULP * (C + 1) * ref)
    assert np.all(got[C == 0] == 0)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['g11', 's1500', 'islands'])
def test_scores_given_weights(name):
    """Fed a host-made W: at alpha = 1 the rows are bitwise the restatement's for windows that do and do not divide
    n_items; at alpha 1.9 and 0.5 within 17 x 2^-52 relative (the two pows); users without items give +0.0 rows,
    excluded columns -inf, out= is honoured, bad user ids are reported by check_indices and the word is cleared."""
    import torch
    from hassaku_amd.data.csr import UserItemCsr
    train, _, _ = _input(name)
    # the same matrix with the items of a few users removed (islands has such users already)
    rows_all = np.repeat(np.arange(train.n_rows), np.diff(train.indptr))
    keep = ~np.isin(rows_all, [0, 7, train.n_rows - 1])
    holed = UserItemCsr.from_pairs(rows_all[keep], train.indices[keep], train.n_rows, train.n_cols)
    m0 = _model(name)
    W, w_u = m0['W'], pr.inv_degrees(np.diff(holed.indptr))
    all_users = np.arange(train.n_rows, dtype=np.int64)
    u = _dev(all_users)
    exp1 = pr.score_rows(all_users, holed.indptr, holed.indices, W, w_u, 1.0)
    m = _model_with(holed, W, w_u, 1.0)
    for w in (7, 64, 100, 1024, 4096):
        m.WINDOW = w
        assert np.array_equal(m.score_rows(u).cpu().numpy(), exp1), w
    zero_rows = m.score_rows(_dev(np.array([0, 7, train.n_rows - 1]))).cpu().numpy()
    assert np.all(zero_rows == 0) and not np.signbit(zero_rows).any()
    # exclusion and out=
    rng = np.random.RandomState(3)
    er_, ec_ = np.nonzero(rng.rand(train.n_rows, train.n_cols) < 0.05)
    excl = UserItemCsr.from_pairs(er_, ec_, train.n_rows, train.n_cols)
    ep, ei = excl.to_device('cuda')
    for alpha in (1.0, 1.9, 0.5):
        exp = exp1 if alpha == 1.0 else pr.score_rows(all_users, holed.indptr, holed.indices, W, w_u, alpha)
        m = _model_with(holed, W, w_u, alpha)
        got = m.score_rows(u).cpu().numpy()
        dist = _rel(got, exp)
        print(f'{name} alpha {alpha}: scores given W, max rel {dist / ULP:.3f} x 2^-52 (bound {0 if alpha == 1 else 17})')
        assert dist <= (0 if alpha == 1.0 else 17 * ULP)
        masked = got.copy()
        masked[er_, ec_] = -np.inf
        for w in (100, 1024):
            m.WINDOW = w
            out = torch.empty((len(all_users), train.n_cols + 2), dtype=torch.float64, device='cuda')
            res = m.score_rows(u, excl=(ep, ei), out=out)
            assert res.data_ptr() == out.data_ptr()
            assert np.array_equal(res.cpu().numpy()[:, :train.n_cols], masked), (alpha, w)
        m.check_indices()
    m = _model_with(holed, W, w_u, 1.9)
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
    partial), an exclusion CSR, alpha = 1.9."""
    import torch
    from hassaku_amd.data.csr import UserItemCsr
    rng = np.random.RandomState(11)
    ur, uc = np.nonzero(rng.rand(5, 70) < 0.3)
    train = UserItemCsr.from_pairs(ur[ur != 3], uc[ur != 3], 5, 70)
    er_, ec_ = np.nonzero(rng.rand(5, 70) < 0.2)
    ep, ei = UserItemCsr.from_pairs(er_, ec_, 5, 70).to_device('cuda')
    m = _model_with(train, rng.rand(70, 70), pr.inv_degrees(np.diff(train.indptr)), 1.9)
    m.WINDOW = 32
    ids = torch.arange(65535 + 3, device='cuda') % 5
    few = m.score_rows(torch.arange(5, device='cuda'), excl=(ep, ei))
    assert torch.isinf(few).any() and bool((few[3][~torch.isinf(few[3])] == 0).all())
    many = m.score_rows(ids, excl=(ep, ei))
    assert many.shape == (65535 + 3, 70) and torch.equal(many, few[ids])
    m.check_indices()


@pytest.mark.gpu
@pytest.mark.parametrize('name, alpha', FIT_CASES)
def test_fit_scores_ranking_metrics(name, alpha):
    """After fit every score is within rtol(alpha, T_max) of the restatement (and, on g11, of the golden pred) with
    the exact zero pattern; on separated users the top-100 ids and per-user metrics equal the golden's (g11) or the
    restatement's (s1500); at most 1 % of the users may be unseparated.  islands checks scores and pattern only: its
    zeros tie."""
    import torch
    from hassaku_amd import hip_ops
    from hassaku_amd.algorithms.graph_algs import P3alpha
    train, val, users = _input(name)
    m0, r = _model(name), _restated(name, alpha)
    m = P3alpha(alpha)
    m.fit(train)
    assert np.array_equal(m.weights(), m.W.cpu().numpy()) and m.weights().shape == (train.n_cols, train.n_cols)
    assert np.array_equal(m.inv_deg_u.cpu().numpy(), m0['w_u'])
    u = _dev(users)
    S = m.score_rows(u).cpu().numpy()
    assert np.array_equal(S == 0, m0['T'] == 0)
    bound = pr.rtol(alpha, m0['t_max'])
    got = _rel(S, r['S'])
    print(f'{name} alpha {alpha}: fitted scores vs restatement {got:.3e}, bound {bound:.3e} (T_max {m0["t_max"]})')
    assert got <= bound
    if name == 'g11':
        g = _gold(alpha)
        got_g = _rel(S, g['pred'])
        print(f'{name} alpha {alpha}: fitted scores vs reference pred {got_g:.3e}, bound {bound:.3e}')
        assert got_g <= bound
    if name == 'islands':
        return
    ok = pr.separated(r['masked'])
    print(f'{name} alpha {alpha}: {int((~ok).sum())} of {len(users)} users unseparated')
    assert (~ok).sum() <= 0.01 * len(users)
    ep, ei = train.to_device('cuda')
    ids = hip_ops.knn_topk_rows(m.score_rows(u, excl=(ep, ei)), 100)[1]
    lp, li = val.to_device('cuda')
    met = hip_ops.rank_metrics(ids, u, lp, li, KS).cpu().numpy()
    ids = ids.cpu().numpy()
    if name == 'g11':
        ref_ids = g['top_ids']
        names = list(g['metric_names'])
        ref_met = {nm: g['metrics'][:, names.index(nm)] for nm in names}
    else:
        _, ref_ids = kr.masked_topk(r['S'], [train.row(int(x)) for x in users])
        ref_met = kr.rank_metrics(ref_ids, [val.row(int(x)) for x in users], ks=tuple(KS))
    assert np.array_equal(ids[ok], ref_ids[ok])
    for t, kk in enumerate(KS):
        for j, nm in enumerate(('precision', 'recall', 'ndcg')):
            np.testing.assert_allclose(met[ok, t, j], ref_met[f'{nm}@{kk}'][ok], rtol=1e-6, atol=1e-7,
                                       err_msg=f'{nm}@{kk}')
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_fit_refuses_what_does_not_fit():
    from hassaku_amd.algorithms.graph_algs import P3alpha
    from hassaku_amd.data.csr import UserItemCsr
    n_items = 400_000                      # W alone would take 1.28 TB
    huge = UserItemCsr.from_pairs(np.arange(10), np.arange(10) * 7, 10, n_items)
    m = P3alpha()
    with pytest.raises(ValueError, match='needs .* bytes of device memory, .* are free'):
        m.fit(huge)
    assert m.W is None


@pytest.mark.gpu
def test_save_load_score_rows_stable(tmp_path):
    from hassaku_amd.algorithms.graph_algs import P3alpha
    train, _, _ = _input('g11')
    m = P3alpha(0.5)
    m.fit(train)
    u = _dev(np.arange(train.n_rows, dtype=np.int64))
    ep, ei = train.to_device('cuda')
    before, before_x = m.score_rows(u).cpu().numpy(), m.score_rows(u, excl=(ep, ei)).cpu().numpy()
    m.save_model_to_path(str(tmp_path))
    with np.load(os.path.join(tmp_path, 'model.npz')) as f:
        assert str(f['alg']) == 'p3alpha' and float(f['alpha']) == 0.5 and f['W'].shape == (train.n_cols, train.n_cols)
        assert int(f['n_users']) == train.n_rows and int(f['n_items']) == train.n_cols and 'pred_mtx' not in f
        assert np.array_equal(f['train_indptr'], train.indptr) and np.array_equal(f['train_indices'], train.indices)
    m2 = P3alpha()                        # alpha comes from the file
    m2.load_model_from_path(str(tmp_path))
    assert m2.alpha == 0.5
    assert np.array_equal(m2.score_rows(u).cpu().numpy(), before)
    assert np.array_equal(m2.score_rows(u, excl=(ep, ei)).cpu().numpy(), before_x)
    # the reference's form, made dense: a 2-D float pred_mtx
    os.makedirs(tmp_path / 'ref')
    np.savez(os.path.join(tmp_path, 'ref', 'model.npz'), pred_mtx=before)
    m3 = P3alpha(0.5)
    m3.load_model_from_path(str(tmp_path / 'ref'))
    assert np.array_equal(m3.score_rows(u).cpu().numpy(), before)
    assert np.array_equal(m3.score_rows(u, excl=(ep, ei)).cpu().numpy(), before_x)
    m3.check_indices()


@pytest.mark.gpu
def test_run_train_val_test(tmp_path):
    """run_experiment's path with -a p3alpha: conf -> slot -> fit -> val metrics -> model.npz -> test metrics through
    load_model_from_path; both equal FullEvaluator fed the restatement's scores.  An unseparated user may rank
    differently, so each such user widens the bound on a mean by 1 / (size of the smallest group)."""
    import torch
    from hassaku_amd.algorithms.algorithms_utils import AlgorithmsEnum
    from hassaku_amd.data.csr import UserItemCsr
    from hassaku_amd.data.data_utils import DatasetsEnum
    from hassaku_amd.data.synthetic import generate, write_csv_dataset
    from hassaku_amd.eval.eval import FullEvaluator
    from hassaku_amd.experiment_helper import run_train_val_test
    d = generate(250, 180, 6000, seed=7, n_groups=2)
    write_csv_dataset(d, str(tmp_path / 'data' / 'ml100k' / 'processed_dataset'))
    conf = {'data_path': str(tmp_path / 'data'), 'model_save_path': str(tmp_path / 'models'), 'alpha': 1.9,
            'eval_batch_size': 64, 'running_settings': {'use_wandb': False, 'batch_verbose': False}}
    best, test, conf = run_train_val_test(AlgorithmsEnum['p3alpha'], DatasetsEnum.ml100k, conf)
    assert os.path.isfile(os.path.join(conf['model_path'], 'model.npz'))
    train = UserItemCsr.from_pairs(d.train[:, 0], d.train[:, 1], d.n_users, d.n_items)
    X = kr.dense_binary(train.indptr, train.indices, d.n_users, d.n_items)
    w_u, w_i = pr.inv_degrees(X.sum(1)), pr.inv_degrees(X.sum(0))
    users = np.arange(d.n_users)
    S = pr.score_rows(users, train.indptr, train.indices, pr.weights(pr.gram(X, w_u), w_i), w_u, 1.9)
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
        ok = pr.separated(masked)
        print(f'{split}: {int((~ok).sum())} of {d.n_users} users unseparated')
        assert (~ok).sum() <= 0.01 * d.n_users
        ev = FullEvaluator(aggr_by_group=True, n_groups=2, user_to_user_group=groups)
        ev.eval_batch(torch.from_numpy(users), torch.from_numpy(masked), torch.from_numpy(labels))
        ref = ev.get_results()
        assert set(ref) <= set(got) and len(ref) == 36
        for name, v in ref.items():
            assert abs(got[name] - v) <= 1e-6 + (~ok).sum() / smallest, (split, name, got[name], v)
