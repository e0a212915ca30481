"""What the seven closed-form models share (FittedRecommenderAlgorithm, ItemWeightAlgorithm, FactorAlgorithm): the keys
and dtypes of every model.npz, every loader refusing every other model's file, the row-block size of the shared count
loop (CPU: hand-made state on device='cpu', nothing here launches a kernel); EASE and SLIM fitted over several count
blocks equal to the bit what one block gives (GPU)."""
import os

import numpy as np
import pytest

# key -> (dtype, number of dimensions) of the model.npz each class wrote before the models were given common bases
NPZ = {
    'iknn': {'alg': ('<U4', 0), 'k': ('<i8', 0), 'n_users': ('<i8', 0), 'n_items': ('<i8', 0),
             'neigh_indptr': ('<i8', 1), 'neigh_indices': ('<i4', 1), 'neigh_data': ('<f8', 1),
             'train_indptr': ('<i8', 1), 'train_indices': ('<i4', 1)},
    'uknn': {'alg': ('<U4', 0), 'k': ('<i8', 0), 'n_users': ('<i8', 0), 'n_items': ('<i8', 0),
             'neigh_indptr': ('<i8', 1), 'neigh_indices': ('<i4', 1), 'neigh_data': ('<f8', 1),
             'train_indptr': ('<i8', 1), 'train_indices': ('<i4', 1)},
    'ease': {'alg': ('<U4', 0), 'lam': ('<f8', 0), 'n_users': ('<i8', 0), 'n_items': ('<i8', 0), 'B': ('<f8', 2),
             'train_indptr': ('<i8', 1), 'train_indices': ('<i4', 1)},
    'slim': {'alg': ('<U4', 0), 'alpha': ('<f8', 0), 'l1_ratio': ('<f8', 0), 'max_iter': ('<i8', 0),
             'n_users': ('<i8', 0), 'n_items': ('<i8', 0), 'W': ('<f8', 2), 'train_indptr': ('<i8', 1),
             'train_indices': ('<i4', 1)},
    'p3alpha': {'alg': ('<U7', 0), 'alpha': ('<f8', 0), 'n_users': ('<i8', 0), 'n_items': ('<i8', 0), 'W': ('<f8', 2),
                'train_indptr': ('<i8', 1), 'train_indices': ('<i4', 1)},
    'svd': {'users_factors': ('<f8', 2), 'items_factors': ('<f8', 2), 'alg': ('<U3', 0), 'n_factors': ('<i8', 0),
            'singular_values': ('<f8', 1)},
    'als': {'users_factors': ('<f8', 2), 'items_factors': ('<f8', 2), 'alg': ('<U3', 0), 'alpha': ('<f8', 0),
            'factors': ('<i8', 0), 'regularization': ('<f8', 0), 'n_iterations': ('<i8', 0)},
}
SCALARS = {'iknn': dict(k=3), 'uknn': dict(k=3), 'ease': dict(lam=5.0), 'slim': dict(alpha=0.02, l1_ratio=0.25, max_iter=9),
           'p3alpha': dict(alpha=0.75), 'svd': dict(n_factors=2),
           'als': dict(alpha=40.0, factors=2, regularization=0.1, n_iterations=3)}
PRED_MTX_LOADERS = ('iknn', 'uknn', 'ease', 'slim', 'p3alpha')     # the reference's file is a dense pred_mtx
FACTOR_LOADERS = ('svd', 'als')                                    # ... or the two factor blocks
STATE = ('pred_mtx', 'train', 'n_users', 'n_items', 'neigh', 'B', 'W', 'inv_deg_u', 'users_factors', 'items_factors',
         'singular_values')
PTR, IDX = np.array([0, 2, 2, 5, 6], np.int64), np.array([0, 3, 1, 2, 4, 0], np.int32)     # 4 users x 5 items


def _new(alg):
    """A model of the class registered as `alg` on device='cpu', without a fit."""
    from hassaku_amd.algorithms.graph_algs import P3alpha
    from hassaku_amd.algorithms.knn_algs import ItemKNN, UserKNN
    from hassaku_amd.algorithms.linear_algs import EASE, SLIM
    from hassaku_amd.algorithms.mf_algs import AlternatingLeastSquare, SVDAlgorithm
    return {'iknn': lambda: ItemKNN('cosine', 3, device='cpu'), 'uknn': lambda: UserKNN('cosine', 3, device='cpu'),
            'ease': lambda: EASE(5, device='cpu'), 'slim': lambda: SLIM(0.02, 0.25, 9, device='cpu'),
            'p3alpha': lambda: P3alpha(0.75, device='cpu'), 'svd': lambda: SVDAlgorithm(2, device='cpu'),
            'als': lambda: AlternatingLeastSquare(40.0, 2, 0.1, 3, device='cpu')}[alg]()


def _hand_made(alg):
    import torch
    t = torch.from_numpy
    m = _new(alg)
    rng = np.random.RandomState(7)
    W, uf, vf = rng.rand(5, 5), rng.standard_normal((4, 2)), rng.standard_normal((5, 2))
    n_ent = 5 if alg == 'iknn' else 4
    neigh = (t(np.arange(n_ent + 1, dtype=np.int64)), t(((np.arange(n_ent) + 1) % n_ent).astype(np.int32)),
             t(rng.rand(n_ent)))
    own = {'iknn': dict(neigh=neigh), 'uknn': dict(neigh=neigh), 'ease': dict(B=t(W)), 'slim': dict(W=t(W)),
           'p3alpha': dict(W=t(W), inv_deg_u=t(np.array([0.5, 0, 1 / 3, 1.]))),
           'svd': dict(users_factors=t(uf), items_factors=t(vf), singular_values=np.array([2., 1.])),
           'als': dict(users_factors=t(uf), items_factors=t(vf))}[alg]
    m.n_users, m.n_items = 4, 5
    if alg not in FACTOR_LOADERS:
        m.train = (t(PTR), t(IDX))
    for key, value in own.items():
        setattr(m, key, value)
    return m


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    """name -> directory of a model.npz: the seven models' own files and the reference's two forms."""
    out = {}
    for name in list(NPZ) + ['ref_pred_mtx', 'ref_factors']:
        out[name] = str(tmp_path_factory.mktemp(name))
    for alg in NPZ:
        _hand_made(alg).save_model_to_path(out[alg])
    rng = np.random.RandomState(8)
    np.savez(os.path.join(out['ref_pred_mtx'], 'model.npz'), pred_mtx=rng.standard_normal((4, 5)))
    np.savez(os.path.join(out['ref_factors'], 'model.npz'), users_factors=rng.standard_normal((4, 2)),
             items_factors=rng.standard_normal((5, 2)))
    return out


@pytest.mark.parametrize('alg', list(NPZ))
def test_model_npz_keys_and_dtypes(files, alg):
    with np.load(os.path.join(files[alg], 'model.npz'), allow_pickle=False) as f:
        assert {k: (f[k].dtype.str, f[k].ndim) for k in f.files} == NPZ[alg]
        assert list(f.files) == list(NPZ[alg])
        assert str(f['alg']) == alg
        for key, value in SCALARS[alg].items():
            assert f[key] == value, key


def _own_format(loader, name):
    return name == loader or name == ('ref_factors' if loader in FACTOR_LOADERS else 'ref_pred_mtx')


@pytest.mark.parametrize('loader', list(NPZ))
def test_every_other_models_file_is_refused(files, loader):
    """A loader that holds a model is handed every file that is not its own format: ValueError, and no model left."""
    import torch
    refused = 0
    for name, path in files.items():
        m = _new(loader)
        m.load_model_from_path(files[loader])
        assert (m.n_users, m.n_items) == (4, 5) and any(getattr(m, attr, None) is not None for attr in STATE[4:])
        if _own_format(loader, name):
            m.load_model_from_path(path)
            assert (m.n_users, m.n_items) == (4, 5)
            continue
        with pytest.raises(ValueError):
            m.load_model_from_path(path)
        assert all(getattr(m, attr, None) is None for attr in STATE), name
        with pytest.raises(RuntimeError, match='fit'):
            m.score_rows(torch.tensor([0]))
        refused += 1
    assert refused == len(files) - 2


@pytest.mark.parametrize('alg', ['ease', 'slim', 'p3alpha'])
def test_item_weight_models_refuse_alike(files, alg, tmp_path):
    """What the three copies did differently: "not fitted" is raised before the user ids are touched, and a matrix of
    a non-float dtype or of another shape is refused with one message."""
    with pytest.raises(RuntimeError, match=r'run fit\(\) or load_model_from_path\(\) first'):
        _new(alg).score_rows(None)
    key = 'B' if alg == 'ease' else 'W'
    with np.load(os.path.join(files[alg], 'model.npz'), allow_pickle=False) as f:
        good = {k: f[k] for k in f.files}
    for bad, said in ((good[key].astype(np.int64), r'int64 \(5, 5\)'), (good[key][:, :4], r'float64 \(5, 4\)'),
                      (good[key].astype(np.float32)[:4], r'float32 \(4, 5\)')):
        np.savez(os.path.join(tmp_path, 'model.npz'), **dict(good, **{key: bad}))
        m = _new(alg)
        with pytest.raises(ValueError, match=rf'{key} of model.npz is {said}, expected floats \(5, 5\)'):
            m.load_model_from_path(str(tmp_path))
        assert all(getattr(m, attr, None) is None for attr in STATE)
    np.savez(os.path.join(tmp_path, 'model.npz'), **dict(good, **{key: good[key].astype(np.float32)}))
    m = _new(alg)
    m.load_model_from_path(str(tmp_path))          # any float dtype is taken and held as float64
    assert np.array_equal(getattr(m, key).numpy(), good[key].astype(np.float32).astype(np.float64))


@pytest.mark.parametrize('gram_block_bytes, n, rows', [
    (1 << 30, 1, 128), (1 << 30, 127, 128), (1 << 30, 128, 128), (1 << 30, 129, 256), (1 << 30, 300, 384),
    (1 << 30, 69878, 3840), (1 << 30, 1 << 20, 256), (1 << 26, 6040, 2688), (1 << 17, 300, 128), (1000, 300, 128),
])
def test_gram_block_rows(gram_block_bytes, n, rows):
    """The rows of one count block, for the three models that walk the int8 Gram: the values the three separate
    expressions gave (n up to a tile, one past it, an odd size, two large ones, a lowered budget, and budgets below one
    128-row block)."""
    for alg in ('iknn', 'ease', 'slim'):
        m = _new(alg)
        assert m.GRAM_BLOCK_BYTES == 1 << 30
        m.GRAM_BLOCK_BYTES = gram_block_bytes
        assert m._gram_block(n) == rows


# ------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize('alg', ['ease', 'slim'])
def test_fit_over_three_count_blocks_is_bitwise_one_block(alg, monkeypatch):
    """60 users x 300 items: with the default budget the Gram loop takes one block of 300 rows, with 128 KiB three
    (128, 128 and 44 rows); the fitted matrix is the same bits."""
    from hassaku_amd import hip_ops
    from hassaku_amd.algorithms.linear_algs import EASE, SLIM
    from hassaku_amd.data.csr import UserItemCsr
    rng = np.random.RandomState(11)
    X = rng.rand(60, 300) < 0.12
    X[:, [3, 299]] = False
    train = UserItemCsr.from_pairs(*np.nonzero(X), 60, 300)
    launched, gram = [], hip_ops.knn_gram_i8
    monkeypatch.setattr(hip_ops, 'knn_gram_i8', lambda M, n, r0, r1, out=None: (launched.append((r0, r1)),
                                                                               gram(M, n, r0, r1, out=out))[1])
    got = []
    for budget, blocks in ((None, [(0, 300)]), (1 << 17, [(0, 128), (128, 256), (256, 300)])):
        m = EASE(5) if alg == 'ease' else SLIM(0.01, 0.3, 50)
        if budget is not None:
            m.GRAM_BLOCK_BYTES = budget
        del launched[:]
        m.fit(train)
        assert launched == blocks
        got.append(m.weights())
    assert got[0].shape == (300, 300) and np.isfinite(got[0]).all() and np.count_nonzero(got[0]) > 300
    assert np.array_equal(got[0], got[1])
