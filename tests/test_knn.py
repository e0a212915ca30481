"""ItemKNN / UserKNN: registry and conf (CPU), the numpy restatement against the reference's goldens (CPU), and the
HIP kernels / model / experiment path against the goldens and the restatement (GPU)."""
import ast
import os
import subprocess
import sys

import numpy as np
import pytest

import knn_restate as kr
from conftest import REPO, load_golden

SIMS = ('cosine', 'jaccard', 'sorensen_dice', 'asymmetric_cosine', 'tversky')
ALGS = ('iknn', 'uknn')
SHRINKS = (0, 10)
CASES = [(a, s, h) for a in ALGS for s in SIMS for h in SHRINKS]


def _data():
    fx = load_golden('g11_knn_data.npz')
    n_users, n_items = int(fx['n_users']), int(fx['n_items'])
    from hassaku_amd.data.csr import UserItemCsr
    train = UserItemCsr.from_pairs(fx['train'][:, 0], fx['train'][:, 1], n_users, n_items)
    val = UserItemCsr.from_pairs(fx['val'][:, 0], fx['val'][:, 1], n_users, n_items)
    return fx, train, val


def _params(sim):
    return ast.literal_eval(str(load_golden('g11_knn_data.npz')['sim_params']))[sim]


def _case(alg, sim, shrink):
    fx = load_golden(f'g11_knn_{alg}_{sim}.npz')
    return {k.split('.', 1)[1]: v for k, v in fx.items() if k.startswith(f's{shrink}.')}


def _entity(train, alg):
    X = kr.dense_binary(train.indptr, train.indices, train.n_rows, train.n_cols)
    return X.T.copy() if alg == 'iknn' else X


def _assert_same_neighbours(mine, g):
    """Row by row: the values equal the reference's bitwise (its self entry of value 0 dropped, divergence 2), the ids
    equal as a set wherever the value is strictly above the row's last kept value (ties: divergence 3)."""
    ptr, idx, dat = mine
    gp, gi, gd = g['neigh_indptr'], g['neigh_indices'], g['neigh_data']
    assert len(ptr) == len(gp)
    for r in range(len(ptr) - 1):
        v, i = dat[ptr[r]:ptr[r + 1]], idx[ptr[r]:ptr[r + 1]]
        tv, ti = gd[gp[r]:gp[r + 1]], gi[gp[r]:gp[r + 1]]
        keep = (ti != r) & (tv > 0)
        tv, ti = tv[keep], ti[keep]
        assert np.array_equal(v, tv), r
        above = v > v[-1] if len(v) else np.zeros(0, bool)
        assert np.array_equal(np.sort(i[above]), np.sort(ti[above])), r     # tie order inside is the reference's own


# ------------------------------------------------------------------------------------------------------ CPU
def test_registry_resolves_knn_slots():
    from hassaku_amd.algorithms.algorithms_utils import ALGORITHM_NAMES, AlgorithmsEnum
    from hassaku_amd.algorithms.knn_algs import ItemKNN, UserKNN
    assert AlgorithmsEnum['iknn'].value is ItemKNN and AlgorithmsEnum['uknn'].value is UserKNN
    assert AlgorithmsEnum.iknn.name == 'iknn' and AlgorithmsEnum.uknn.value is UserKNN
    assert AlgorithmsEnum['mf'] is AlgorithmsEnum.mf
    assert set(ALGORITHM_NAMES) == {m.name for m in AlgorithmsEnum} | {'iknn', 'uknn'}
    with pytest.raises(KeyError):
        AlgorithmsEnum['knn']


def test_cli_lists_knn():
    out = subprocess.run([sys.executable, os.path.join(REPO, 'run_experiment.py'), '--help'], capture_output=True,
                         text=True, cwd=REPO, check=True).stdout
    assert 'iknn' in out and 'uknn' in out


@pytest.mark.parametrize('bad, msg', [
    ({'sim_func_params': {'sim_func_name': 'pearson'}, 'k': 10}, 'not one of'),
    ({'sim_func_params': {'sim_func_name': 'asymmetric_cosine'}, 'k': 10}, 'alpha'),
    ({'sim_func_params': {'sim_func_name': 'tversky', 'alpha': .5}, 'k': 10}, 'beta'),
    ({'sim_func_params': {'sim_func_name': 'cosine'}, 'k': 0}, 'k = 0'),
    ({'sim_func_params': {'sim_func_name': 'cosine'}, 'k': 1025}, 'k = 1025'),
    ({'sim_func_params': {'sim_func_name': 'cosine'}}, 'needs k'),
    ({'k': 5}, 'sim_func_name'),
])
def test_conf_validation(tmp_path, bad, msg):
    from hassaku_amd.algorithms.algorithms_utils import AlgorithmsEnum
    from hassaku_amd.conf.conf_parser import parse_conf
    from hassaku_amd.data.data_utils import DatasetsEnum
    for alg in ('iknn', 'uknn'):
        conf = dict(bad, data_path=str(tmp_path), model_save_path=str(tmp_path / 'm'))
        with pytest.raises(ValueError, match=msg):
            parse_conf(conf, AlgorithmsEnum[alg], DatasetsEnum.ml1m)


def test_conf_gets_no_sgd_defaults(tmp_path):
    from hassaku_amd.algorithms.algorithms_utils import AlgorithmsEnum
    from hassaku_amd.algorithms.knn_algs import ItemKNN, SimilarityFunctionEnum
    from hassaku_amd.conf.conf_parser import parse_conf
    from hassaku_amd.data.data_utils import DatasetsEnum
    conf = {'data_path': str(tmp_path), 'model_save_path': str(tmp_path / 'm'), 'k': 7,
            'sim_func_params': {'sim_func_name': 'tversky', 'alpha': .2, 'beta': .9}}
    conf = parse_conf(conf, AlgorithmsEnum.iknn, DatasetsEnum.ml1m)
    assert 'lr' not in conf and 'n_epochs' not in conf and 'optimizer' not in conf
    m = AlgorithmsEnum.iknn.value.build_from_conf(conf, None)
    assert isinstance(m, ItemKNN) and m.k == 7 and m.shrinkage == 0. and m.sim_func_enum is SimilarityFunctionEnum.tversky
    assert (m.alpha, m.beta) == (.2, .9)
    assert [s.name for s in SimilarityFunctionEnum] == list(SIMS)


def test_model_npz_round_trip(tmp_path):
    import torch
    from hassaku_amd.algorithms.knn_algs import ItemKNN, UserKNN
    m = UserKNN('cosine', 5, device='cpu')
    m.n_users, m.n_items = 3, 4
    m.neigh = (torch.tensor([0, 1, 1, 2]), torch.tensor([2, 0], dtype=torch.int32), torch.tensor([.5, .25],
                                                                                                    dtype=torch.float64))
    m.train = (torch.tensor([0, 2, 3, 4]), torch.tensor([0, 3, 1, 2], dtype=torch.int32))
    m.save_model_to_path(str(tmp_path))
    m2 = UserKNN('cosine', 5, device='cpu')
    m2.load_model_from_path(str(tmp_path))
    assert (m2.n_users, m2.n_items) == (3, 4)
    for a, b in zip(m.neigh + m.train, m2.neigh + m2.train):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match='uknn'):
        ItemKNN('cosine', 5, device='cpu').load_model_from_path(str(tmp_path))
    # the reference's own form: a dense float64 pred_mtx
    pred = np.arange(12, dtype=np.float64).reshape(3, 4) / 7
    np.savez(os.path.join(tmp_path, 'model.npz'), pred_mtx=pred)
    m3 = ItemKNN('cosine', 5, device='cpu')
    m3.load_model_from_path(str(tmp_path))
    got = m3.predict(torch.tensor([2, 0]), torch.tensor([[3, 1], [0, 2]]))
    assert got.dtype == torch.float64
    assert np.array_equal(got.numpy(), np.array([[pred[2, 3], pred[2, 1]], [pred[0, 0], pred[0, 2]]]))
    rows = m3.score_rows(torch.tensor([1]), excl=(torch.tensor([0, 0, 2, 2]), torch.tensor([1, 3], dtype=torch.int32)))
    assert np.array_equal(rows.numpy(), np.array([[pred[1, 0], -np.inf, pred[1, 2], -np.inf]]))


@pytest.mark.parametrize('alg, sim, shrink', CASES)
def test_restatement_equals_reference(alg, sim, shrink):
    """The numpy restatement reproduces the reference bit for bit: similarity values (as multisets per row and per
    value-distinct position), the pred rows fed with the reference's own neighbours, and the masked top-100 values."""
    fx, train, val = _data()
    g = _case(alg, sim, shrink)
    k = int(fx['k'])
    ptr, idx, dat = kr.neighbours(_entity(train, alg), sim, k, float(shrink), **_params(sim))
    _assert_same_neighbours((ptr, idx, dat), g)
    users = fx['users']
    pred = kr.predictions(alg, users, (train.indptr, train.indices),
                          (g['neigh_indptr'], g['neigh_indices'], g['neigh_data']), train.n_rows, train.n_cols)
    assert np.array_equal(pred, g['pred'])
    vals, _ = kr.masked_topk(pred, [train.row(int(u)) for u in users])
    assert np.array_equal(vals, g['top_vals'])


# ------------------------------------------------------------------------------------------------------ GPU
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize('n, d, p_empty', [(333, 1000, 0.1), (517, 777, 0.3), (1100, 70, 0.0)])
def test_gram_exact(n, d, p_empty):
    import torch
    from hassaku_amd import hip_ops
    rng = np.random.RandomState(n)
    M = (rng.rand(n, d) < 0.05).astype(np.float64)
    M[rng.rand(n) < p_empty] = 0.
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(M.sum(1).astype(np.int64), out=ptr[1:])
    ind = np.nonzero(M)[1].astype(np.int32)
    P = hip_ops.knn_pack_i8(_dev(ptr), _dev(ind), n, d)
    ref = (M @ M.T).astype(np.int64)
    for block in (128, 256, 1 << 20):
        for r0 in range(0, n, block):
            r1 = min(r0 + block, n)
            C = hip_ops.knn_gram_i8(P, n, r0, r1)
            torch.cuda.synchronize()
            assert np.array_equal(C.cpu().numpy().astype(np.int64), ref[r0:r1]), (block, r0)


@pytest.mark.gpu
@pytest.mark.parametrize('alg, sim, shrink', CASES)
def test_fit_similarity_bitwise(alg, sim, shrink):
    """Neighbour values equal the reference's bitwise; ids equal wherever the value is strictly above the row's k-th."""
    from hassaku_amd.algorithms.knn_algs import ItemKNN, UserKNN
    fx, train, _ = _data()
    g = _case(alg, sim, shrink)
    m = (ItemKNN if alg == 'iknn' else UserKNN)(sim, int(fx['k']), float(shrink), **_params(sim))
    m.fit(train)
    ptr, idx, dat = m.neighbours()
    _assert_same_neighbours((ptr, idx, dat), g)


@pytest.mark.gpu
@pytest.mark.parametrize('k', [1, 3, 512])
@pytest.mark.parametrize('alg, sim', [('iknn', 'cosine'), ('uknn', 'tversky'), ('iknn', 'asymmetric_cosine'),
                                      ('uknn', 'jaccard')])
def test_fit_neighbours_vs_restatement(alg, sim, k):
    from hassaku_amd.algorithms.knn_algs import ItemKNN, UserKNN
    _, train, _ = _data()
    m = (ItemKNN if alg == 'iknn' else UserKNN)(sim, k, 10., **_params(sim))
    m.fit(train)
    got = m.neighbours()
    exp = kr.neighbours(_entity(train, alg), sim, k, 10., **_params(sim))
    for a, b in zip(got, exp):
        assert np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize('alg', ALGS)
@pytest.mark.parametrize('sim, shrink', [('cosine', 0), ('tversky', 10), ('jaccard', 10)])
def test_scoring_bitwise_with_reference_neighbours(alg, sim, shrink):
    """Fed the reference's own neighbour CSR, the score rows are bitwise its pred rows, for one and for many windows;
    the masked top-100 and the per-user metrics match."""
    import torch
    from hassaku_amd import hip_ops
    from hassaku_amd.algorithms.knn_algs import ItemKNN, UserKNN
    fx, train, val = _data()
    g = _case(alg, sim, shrink)
    m = (ItemKNN if alg == 'iknn' else UserKNN)(sim, int(fx['k']), float(shrink), **_params(sim))
    m.n_users, m.n_items = train.n_rows, train.n_cols
    m.train = (_dev(train.indptr), _dev(train.indices))
    m.neigh = (_dev(g['neigh_indptr']), _dev(g['neigh_indices']), _dev(g['neigh_data']))
    u = _dev(fx['users'])
    full = m.score_rows(u).cpu().numpy()
    assert np.array_equal(full, g['pred'])
    for w in (7, 64, 150):
        m.WINDOW = w
        assert np.array_equal(m.score_rows(u).cpu().numpy(), g['pred']), w
    m.WINDOW = 4096
    ep, ei = train.to_device('cuda')
    scores = m.score_rows(u, excl=(ep, ei))
    vals, ids = hip_ops.knn_topk_rows(scores, 100)
    vals, ids = vals.cpu().numpy(), ids.cpu().numpy()
    assert np.array_equal(vals, g['top_vals'])
    for q in range(len(u)):
        strict = vals[q] > vals[q, -1]
        assert np.array_equal(np.sort(ids[q][strict]), np.sort(g['top_ids'][q][strict])), q   # tie order: theirs
    lp, li = val.to_device('cuda')
    met = hip_ops.rank_metrics(ids_t := torch.from_numpy(ids).cuda(), u, lp, li, [100, 50, 10, 5]).cpu().numpy()
    del ids_t
    names = list(g['metric_names'])
    tv = g['top_vals']
    no_ties = np.all(tv[:, :-1] != tv[:, 1:], axis=1) & g['gap']      # ndcg also depends on the order inside ties
    for t, kk in enumerate([100, 50, 10, 5]):
        cut = g['gap'] if kk == 100 else tv[:, kk - 1] != tv[:, kk]   # the set at the cut-off is the reference's
        for j, nm in enumerate(('precision', 'recall', 'ndcg')):
            ref = g['metrics'][:, names.index(f'{nm}@{kk}')]
            ok = no_ties if nm == 'ndcg' else cut
            np.testing.assert_allclose(met[ok, t, j], ref[ok], rtol=1e-6, atol=1e-7, err_msg=f'{nm}@{kk}')


@pytest.mark.gpu
def test_topk_rows_ties_and_large_k():
    import torch
    from hassaku_amd import hip_ops
    rng = np.random.RandomState(0)
    S = np.round(rng.rand(37, 9000) * 8) / 8          # many ties
    S[3, :] = 0.
    S[5, 100:200] = -np.inf
    for k in (1, 100, 1024):
        v, i = hip_ops.knn_topk_rows(_dev(S), k)
        ids = np.stack([np.lexsort((np.arange(S.shape[1]), -row))[:k] for row in S])
        assert np.array_equal(i.cpu().numpy(), ids) and np.array_equal(v.cpu().numpy(), np.take_along_axis(S, ids, 1))
    with pytest.raises(RuntimeError):
        hip_ops.knn_topk_rows(_dev(S), 1025)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize('alg, sim', [('iknn', 'cosine'), ('uknn', 'asymmetric_cosine')])
def test_ml1m_shape_vs_restatement(alg, sim):
    """ml1m-shaped synthetic set: neighbours, a sample of score rows and their metrics equal the restatement."""
    import torch
    from hassaku_amd import hip_ops
    from hassaku_amd.algorithms.knn_algs import ItemKNN, UserKNN
    from hassaku_amd.data.csr import UserItemCsr
    from hassaku_amd.data.synthetic import generate_named
    d = generate_named('ml1m', seed=2)
    train = UserItemCsr.from_pairs(d.train[:, 0], d.train[:, 1], d.n_users, d.n_items)
    val = UserItemCsr.from_pairs(d.val[:, 0], d.val[:, 1], d.n_users, d.n_items)
    params = {'alpha': .4} if sim == 'asymmetric_cosine' else {}
    m = (ItemKNN if alg == 'iknn' else UserKNN)(sim, 100, 5., **params)
    m.GRAM_BLOCK_BYTES = 1 << 26     # several row blocks
    m.fit(train)
    got = m.neighbours()
    exp = kr.neighbours(_entity(train, alg), sim, 100, 5., **params)
    for a, b in zip(got, exp):
        assert np.array_equal(a, b)
    users = np.sort(np.random.RandomState(1).choice(d.n_users, 24, replace=False))
    pred = kr.predictions(alg, users, (train.indptr, train.indices), exp, d.n_users, d.n_items)
    u = _dev(users)
    assert np.array_equal(m.score_rows(u).cpu().numpy(), pred)
    ep, ei = train.to_device('cuda')
    vals, ids = hip_ops.knn_topk_rows(m.score_rows(u, excl=(ep, ei)), 100)
    ev, eids = kr.masked_topk(pred, [train.row(int(x)) for x in users])
    assert np.array_equal(vals.cpu().numpy(), ev) and np.array_equal(ids.cpu().numpy(), eids)
    lp, li = val.to_device('cuda')
    met = hip_ops.rank_metrics(torch.from_numpy(eids.astype(np.int32)).cuda(), u, lp, li, [100, 10]).cpu().numpy()
    ref = kr.rank_metrics(eids, [val.row(int(x)) for x in users], ks=(100, 10))
    np.testing.assert_allclose(met[:, 1, 2], ref['ndcg@10'], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(met[:, 0, 1], ref['recall@100'], rtol=1e-6, atol=1e-7)


@pytest.mark.gpu
@pytest.mark.parametrize('alg', ALGS)
def test_run_train_val_test(tmp_path, alg):
    """run_experiment's path: conf -> slot -> fit on the train CSR -> val metrics -> model.npz -> test metrics through
    load_model_from_path; both equal the restatement's."""
    from hassaku_amd.algorithms.algorithms_utils import AlgorithmsEnum
    from hassaku_amd.data.csr import UserItemCsr
    from hassaku_amd.data.data_utils import DatasetsEnum
    from hassaku_amd.data.synthetic import generate, write_csv_dataset
    from hassaku_amd.experiment_helper import run_train_val_test
    d = generate(250, 180, 6000, seed=7, n_groups=2)
    write_csv_dataset(d, str(tmp_path / 'data' / 'ml100k' / 'processed_dataset'))
    conf = {'data_path': str(tmp_path / 'data'), 'model_save_path': str(tmp_path / 'models'), 'k': 30, 'shrinkage': 4,
            'sim_func_params': {'sim_func_name': 'jaccard'}, 'eval_batch_size': 64,
            'running_settings': {'use_wandb': False, 'batch_verbose': False}}
    best, test, conf = run_train_val_test(AlgorithmsEnum[alg], DatasetsEnum.ml100k, conf)
    assert os.path.isfile(os.path.join(conf['model_path'], 'model.npz'))
    train = UserItemCsr.from_pairs(d.train[:, 0], d.train[:, 1], d.n_users, d.n_items)
    X = kr.dense_binary(train.indptr, train.indices, d.n_users, d.n_items)
    S = kr.neighbours(X.T.copy() if alg == 'iknn' else X, 'jaccard', 30, 4.)
    users = np.arange(d.n_users)
    pred = kr.predictions(alg, users, (train.indptr, train.indices), S, d.n_users, d.n_items)
    for split, got in (('val', best), ('test', test)):
        excl_pairs = d.train if split == 'val' else np.concatenate([d.train, d.val])
        excl = UserItemCsr.from_pairs(excl_pairs[:, 0], excl_pairs[:, 1], d.n_users, d.n_items)
        lab_pairs = getattr(d, split)
        lab = UserItemCsr.from_pairs(lab_pairs[:, 0], lab_pairs[:, 1], d.n_users, d.n_items)
        _, ids = kr.masked_topk(pred, [excl.row(int(u)) for u in users])
        ref = kr.rank_metrics(ids, [lab.row(int(u)) for u in users])
        for name, v in ref.items():
            assert abs(got[name] - v.mean()) <= 1e-6, (split, name, got[name], v.mean())
