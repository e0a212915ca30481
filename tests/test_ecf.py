"""ECF: registry, conf, tag dataset, seeded construction, state dicts and the restatements against the reference's g17
golden (CPU); the affiliation kernels against tests/ecf_restate.py, one training step and the evaluation scores against
the golden, memory and the experiment path (GPU).

Bounds.  The operator is compared with the float64 restatement; it may miss it by 4 x what the same formulas evaluated
in float32 on the CPU miss it by on the same input (the margin of tests/test_eval_structured.py for a device fp32 path
against an fp32 form), or 1e-6, per row and relative to the row's largest magnitude in the float64 result.  The model is
compared with the golden by max_norm_err; the bound is 4 x the reference's own distance from the float64 restatement,
which the golden stores per quantity, or 1e-5 (the README's fp32 golden parity).  The discrete choices (top-k masks,
top-p tags) are at least 1e-4 clear of a flip in the golden (`gap.*`), so they are compared exactly.  Every test that
uses a bound prints it with the measured value.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ecf_restate
from conftest import REPO, load_golden, max_norm_err

BLOCKS = ('c24', 'c64')
QUANTITIES = ('x_tilde', 'xs', 'a', 'scores', 'cf_loss', 'ind_loss', 'ts_loss', 'grad.clusters',
              'grad.user_embed.weight', 'grad.item_embed.weight', 'eval.scores')
KEYS = ('clusters', 'item_embed.weight', 'user_embed.weight')


@functools.lru_cache(maxsize=None)
def _gold():
    return load_golden('g17_ecf.npz')


@functools.lru_cache(maxsize=None)
def _g11():
    return load_golden('g11_knn_data.npz')


@functools.lru_cache(maxsize=None)
def _train_csr():
    from hassaku_amd.data.csr import UserItemCsr
    fx = _g11()
    return UserItemCsr.from_pairs(fx['train'][:, 0], fx['train'][:, 1], int(fx['n_users']), int(fx['n_items']))


def _tag_matrix():
    from scipy import sparse as sp
    return sp.csr_matrix(_gold()['tag_matrix'])


def _hyper(block):
    fx = _gold()
    return dict(embedding_dim=int(fx['embedding_dim']), n_clusters=int(fx[f'{block}.n_clusters']),
                top_n=int(fx[f'{block}.top_n']), top_m=int(fx[f'{block}.top_m']), top_p=int(fx['top_p']),
                temp_masking=float(fx['temp_masking']), temp_tags=float(fx['temp_tags']))


def _gold_model(block='c24', seed=None):
    from hassaku_amd.algorithms.ecf_alg import ECF
    fx = _gold()
    torch.manual_seed(int(fx[f'{block}.model_seed']) if seed is None else seed)
    return ECF(int(fx['n_users']), int(fx['n_items']), _tag_matrix(), _train_csr(), **_hyper(block))


def _init_state(block):
    return {k: torch.from_numpy(_gold()[f'{block}.init.{k}']) for k in KEYS}


def _write_dataset(path, extra_tag=False):
    """The g11 dataset with the golden's tag files; extra_tag appends a tag no item carries."""
    import pandas as pd
    from hassaku_amd.data.synthetic import generate, write_csv_dataset
    fx = _gold()
    data = generate(300, 200, 6000, seed=11, n_groups=2)
    assert np.array_equal(data.train, _g11()['train'])
    write_csv_dataset(data, path)
    n_tags = int(fx['n_tags']) + int(extra_tag)
    pd.DataFrame({'tag_idx': np.arange(n_tags)}).to_csv(os.path.join(path, 'tag_idxs.csv'), index=False)
    pd.DataFrame({'item_idx': fx['item_tag'][:, 0], 'tag_idx': fx['item_tag'][:, 1]}).to_csv(
        os.path.join(path, 'item_tag_idxs.csv'), index=False)


# ------------------------------------------------------------------------------------------------------ CPU
def test_registry_resolves_ecf():
    from hassaku_amd.algorithms import algorithms_utils as au
    from hassaku_amd.algorithms.base_classes import SGDBasedRecommenderAlgorithm
    from hassaku_amd.algorithms.ecf_alg import ECF
    assert au.AlgorithmsEnum['ecf'].value is ECF and au.AlgorithmsEnum.ecf.name == 'ecf'
    assert au.AlgorithmsEnum['ecf'] is au.TagAlgorithmsEnum.ecf
    assert [m.name for m in au.TagAlgorithmsEnum] == ['ecf']
    assert issubclass(ECF, SGDBasedRecommenderAlgorithm)
    assert au.RUNNABLE_ALGORITHM_NAMES == au.EXPERIMENT_ALGORITHM_NAMES + ('ecf',)
    # the older objects are what they were
    assert [m.name for m in au.AlgorithmsEnum] == ['mf', 'sgdbias', 'uprotomf', 'iprotomf', 'uiprotomf', 'acf']
    assert [m.name for m in au.NeuralAlgorithmsEnum] == ['dmf']
    assert au.ALGORITHM_NAMES == ('mf', 'sgdbias', 'uprotomf', 'iprotomf', 'uiprotomf', 'acf', 'uknn', 'iknn')
    assert au.ALL_ALGORITHM_NAMES == au.ALGORITHM_NAMES + ('ease',)
    assert au.REGISTERED_ALGORITHM_NAMES == au.ALL_ALGORITHM_NAMES + ('p3alpha',)
    assert au.CLI_ALGORITHM_NAMES == au.REGISTERED_ALGORITHM_NAMES + ('svd',)
    assert au.EXPERIMENT_ALGORITHM_NAMES == au.CLI_ALGORITHM_NAMES + ('dmf',)
    for missing in ('slim', 'rp3beta', 'knn', 'als', 'rbmf', 'pop', 'rand'):
        with pytest.raises(KeyError):
            au.AlgorithmsEnum[missing]


def test_cli_lists_ecf():
    out = subprocess.run([sys.executable, os.path.join(REPO, 'run_experiment.py'), '--help'], capture_output=True,
                         text=True, cwd=REPO, check=True).stdout
    assert 'ecf' in out and 'dmf' in out and 'svd' in out and 'iknn' in out


@pytest.mark.parametrize('change, msg', [
    ({'n_clusters': 24.0}, 'n_clusters must be an int'),
    ({'n_clusters': True}, 'n_clusters must be an int'),
    ({'top_n': '5'}, 'top_n must be an int'),
    ({'top_m': 2.5}, 'top_m must be an int'),
    ({'top_p': False}, 'top_p must be an int'),
    ({'embedding_dim': 20.0}, 'embedding_dim must be an int'),
    ({'n_clusters': 0}, r'n_clusters must be in \[1, 64\]'),
    ({'n_clusters': 65, 'top_n': 5, 'top_m': 5}, r'n_clusters must be in \[1, 64\]'),
    ({'n_clusters': 24, 'top_n': 0}, r'top_n must be in \[1, n_clusters = 24\]'),
    ({'n_clusters': 24, 'top_n': 25}, r'top_n must be in \[1, n_clusters = 24\]'),
    ({'n_clusters': 24, 'top_m': 0, 'top_n': 5}, r'top_m must be in \[1, n_clusters = 24\]'),
    ({'n_clusters': 24, 'top_m': 25, 'top_n': 5}, r'top_m must be in \[1, n_clusters = 24\]'),
    ({'n_clusters': 16}, r'top_n must be in \[1, n_clusters = 16\]'),          # the default top_n = 20
    ({'top_p': 0}, r'top_p must be in \[1, n_tags\]'),
    ({'temp_masking': 0}, 'temp_masking must be a positive number'),
    ({'temp_masking': -2.}, 'temp_masking must be a positive number'),
    ({'temp_tags': 0.}, 'temp_tags must be a positive number'),
    ({'temp_tags': '2'}, 'temp_tags must be a positive number'),
    ({'temp_tags': float('nan')}, 'temp_tags must be a positive number'),
])
def test_conf_validation(tmp_path, change, msg):
    from hassaku_amd.algorithms.algorithms_utils import AlgorithmsEnum
    from hassaku_amd.conf.conf_parser import parse_conf, validate_ecf_conf
    from hassaku_amd.data.data_utils import DatasetsEnum
    with pytest.raises(ValueError, match=msg):
        validate_ecf_conf(dict(change))
    conf = dict(change, data_path=str(tmp_path), model_save_path=str(tmp_path / 'm'))
    with pytest.raises(ValueError, match=msg):
        parse_conf(conf, AlgorithmsEnum.ecf, DatasetsEnum.ml100k)


def test_conf_defaults_build_and_size_checks(tmp_path):
    from hassaku_amd.algorithms.algorithms_utils import AlgorithmsEnum
    from hassaku_amd.algorithms.ecf_alg import ECF
    from hassaku_amd.conf.conf_parser import parse_conf
    from hassaku_amd.data.data_utils import DatasetsEnum, get_dataloader
    from hassaku_amd.data.dataset import ECFTrainRecDataset
    conf = parse_conf({'data_path': str(tmp_path), 'model_save_path': str(tmp_path / 'm'), 'embedding_dim': 8},
                      AlgorithmsEnum.ecf, DatasetsEnum.ml100k)
    assert conf['alg'] == 'ecf' and conf['rec_loss'] == 'bce' and conf['neg_train'] == 4
    assert 'n_clusters' not in conf                   # the model's own defaults are filled where it is built
    _write_dataset(conf['dataset_path'])
    train = get_dataloader(dict(conf, device='cpu'), 'train').dataset
    assert isinstance(train, ECFTrainRecDataset)
    model = AlgorithmsEnum.ecf.value.build_from_conf(conf, train)
    assert (model.embedding_dim, model.n_clusters, model.top_n, model.top_m, model.top_p) == (8, 64, 20, 20, 4)
    assert (model.temp_masking, model.temp_tags, model.lam_cf, model.lam_ind, model.lam_ts) == (2., 2., .6, 1., 1.)
    assert model.name == 'ECF' and model.n_tags == 12
    assert torch.equal(model.x_indices, torch.from_numpy(train.sampling_csr.indices))
    # the same model from the weighted matrix alone
    other = ECF(train.n_users, train.n_items, train.tag_matrix, train.sampling_matrix, 8)
    for name in ('tag_indptr', 'tag_indices', 'tag_weight', 'x_indptr', 'x_indices'):
        assert torch.equal(getattr(other, name), getattr(model, name)), name
    # what depends on the sizes is checked by the constructor
    with pytest.raises(ValueError, match=r'top_p must be in \[1, n_tags = 12\]'):
        AlgorithmsEnum.ecf.value.build_from_conf(dict(conf, top_p=13), train)
    small = _train_csr().to_scipy(np.int16)[:, :30]
    with pytest.raises(ValueError, match=r'n_clusters must be in \[1, 30\]'):
        ECF(300, 30, _tag_matrix()[:30], small, 8, n_clusters=31, top_n=5, top_m=5)
    with pytest.raises(ValueError, match='interaction_matrix has shape'):
        ECF(300, 200, _tag_matrix(), small, 8)
    with pytest.raises(ValueError, match='expected 200 rows'):
        ECF(300, 200, _tag_matrix()[:30], _train_csr(), 8)
    uneven = _tag_matrix().tolil()
    uneven[np.nonzero(_gold()['tag_matrix'][:, 3])[0][0], 3] *= 2
    with pytest.raises(ValueError, match='column 3 are not constant'):
        ECF(300, 200, uneven.tocsr(), _train_csr(), 8)


def test_tag_dataset_is_the_reference_s(tmp_path):
    from hassaku_amd.data.dataset import ECFTrainRecDataset
    fx = _gold()
    _write_dataset(str(tmp_path / 'a'))
    data = ECFTrainRecDataset(str(tmp_path / 'a'))
    dense = data.tag_matrix.toarray()
    assert dense.dtype == np.float64 and dense.shape == (200, 12)
    assert np.array_equal(dense, fx['tag_matrix'])                      # bit for bit
    assert data.tag_incidence.dtype == np.int16 and data.tag_weight.shape == (12,) and data.n_tags == 12
    assert np.array_equal(data.tag_incidence.toarray() * data.tag_weight[None, :], dense)
    assert (data.tag_incidence.toarray().sum(1) == 0).any()             # items without a tag
    assert len(data) == len(_g11()['train']) and data.n_items == 200
    _write_dataset(str(tmp_path / 'b'), extra_tag=True)
    wider = ECFTrainRecDataset(str(tmp_path / 'b'))
    assert wider.tag_matrix.shape == (200, 13) and np.array_equal(wider.tag_matrix.toarray()[:, :12], dense)
    assert wider.tag_weight[12] == np.log(200 / 1e-6) and np.isfinite(wider.tag_weight).all()
    assert wider.tag_weight[12] > 2 * wider.tag_weight[:12].max()


@pytest.mark.parametrize('block', BLOCKS)
def test_seeded_construction_is_the_reference_s(block):
    sd = _gold_model(block).state_dict()
    assert sorted(sd) == sorted(KEYS)
    for k, v in _init_state(block).items():
        assert tuple(sd[k].shape) == tuple(v.shape), k
        assert torch.equal(sd[k], v), k
    # the clusters are rows of the item table
    items = sd['item_embed.weight']
    assert all((items == row).all(1).any() for row in sd['clusters'])


def test_state_dict_round_trip_and_reference_written_dicts(tmp_path):
    model, other = _gold_model(), _gold_model(seed=1)
    sd = model.state_dict()
    assert not torch.equal(other.state_dict()['clusters'], sd['clusters'])
    other.load_state_dict(sd)
    assert all(torch.equal(v, sd[k]) for k, v in other.state_dict().items())
    model.save_model_to_path(str(tmp_path))
    assert sorted(torch.load(os.path.join(str(tmp_path), 'model.pth'))) == sorted(KEYS)
    third = _gold_model(seed=2)
    third.load_model_from_path(str(tmp_path))
    assert all(torch.equal(v, sd[k]) for k, v in third.state_dict().items())
    # non-strict from disk, as the reference's: a checkpoint without the clusters leaves them alone
    os.makedirs(str(tmp_path / 'partial'))
    torch.save({k: v for k, v in sd.items() if k != 'clusters'}, os.path.join(str(tmp_path / 'partial'), 'model.pth'))
    fourth = _gold_model(seed=3)
    before = fourth.clusters.detach().clone()
    fourth.load_model_from_path(str(tmp_path / 'partial'))
    assert torch.equal(fourth.clusters, before) and torch.equal(fourth.item_embed.weight, sd['item_embed.weight'])
    # a reference-written dict with its two dense matrices
    ref_sd = dict(sd, tag_matrix=torch.from_numpy(_gold()['tag_matrix']).float(),
                  interaction_matrix=torch.from_numpy(_train_csr().to_scipy(np.float32).toarray()))
    fifth = _gold_model(seed=4)
    res = fifth.load_state_dict(ref_sd)
    assert not res.missing_keys and not res.unexpected_keys and len(ref_sd) == 5
    assert all(torch.equal(v, sd[k]) for k, v in fifth.state_dict().items())
    for key in ('tag_matrix', 'interaction_matrix'):
        with pytest.raises(ValueError, match=key):
            fifth.load_state_dict(dict(ref_sd, **{key: ref_sd[key].T.contiguous()}))
    with pytest.raises(RuntimeError, match='clusters'):
        fifth.load_state_dict(dict(sd, clusters=sd['clusters'].T.contiguous()))


def test_holds_no_dense_matrix():
    model = _gold_model('c64')
    U, I, T = model.n_users, model.n_items, model.n_tags
    assert (U, I, T) == (300, 200, 12)
    names = {n for n, _ in model.named_buffers()}
    assert names == {'x_indptr', 'x_indices', 'tag_indptr', 'tag_indices', 'tag_weight', 'tag_rows'}
    assert not any(n in names for n in model.state_dict())
    tensors = list(model.parameters()) + list(model.buffers()) + [v for v in vars(model).values() if torch.is_tensor(v)]
    assert len(tensors) >= 9
    for t in tensors:
        assert t.numel() not in (U * I, I * T) and t.numel() <= max(U, I) * model.embedding_dim
    # the buffers are X by rows and the incidence by tags
    X = _train_csr().to_scipy(np.float64).toarray()
    back = np.zeros((U, I))
    back[np.repeat(np.arange(U), np.diff(model.x_indptr.numpy())), model.x_indices.numpy()] = 1
    assert np.array_equal(back, X)
    inc = np.zeros((T, I))
    inc[np.repeat(np.arange(T), np.diff(model.tag_indptr.numpy())), model.tag_indices.numpy()] = 1
    assert np.array_equal(inc.T * model.tag_weight.numpy()[None, :], _gold()['tag_matrix'].astype(np.float32))


def _restated(block):
    """The float64 restatement on the golden's initial state and batch: {quantity: numpy}."""
    fx = _gold()
    leaves = {k: v.double().requires_grad_() for k, v in _init_state(block).items()}
    X = torch.from_numpy(_train_csr().to_scipy(np.float64).toarray())
    T = torch.from_numpy(fx['tag_matrix'])
    h = _hyper(block)
    args = (leaves['user_embed.weight'], leaves['item_embed.weight'], leaves['clusters'], X, T)
    hyper = (h['top_n'], h['top_m'], h['temp_masking'], h['temp_tags'], h['top_p'])
    r = ecf_restate.forward_f64(*args, torch.from_numpy(fx[f'{block}.u_idx']), torch.from_numpy(fx[f'{block}.i_idx']),
                                *hyper)
    lam_cf, lam_ind, lam_ts = fx['lam']
    out = {'x_tilde': r['x_tilde'], 'xs': r['xs'], 'a': r['a'], 'scores': r['scores'], 'cf_loss': lam_cf * r['cf'],
           'ind_loss': lam_ind * r['ind'], 'ts_loss': lam_ts * r['ts']}
    (ecf_restate.bpr(r['scores']) + out['cf_loss'] + out['ind_loss'] + out['ts_loss']).backward()
    out = {k: v.detach().numpy() for k, v in out.items()}
    for k, leaf in leaves.items():
        out['grad.' + k] = leaf.grad.numpy()
    with torch.no_grad():
        out['eval.scores'] = ecf_restate.forward_f64(*args, torch.from_numpy(fx['eval.u']),
                                                     torch.arange(int(fx['n_items'])), *hyper)['scores'].numpy()
    return out


@pytest.mark.parametrize('block', BLOCKS)
def test_restatement_reproduces_the_golden_within_the_stored_distances(block):
    fx = _gold()
    want = _restated(block)
    for q in QUANTITIES:
        dist = float(fx[f'{block}.dist.{q}'])
        e = max_norm_err(fx[f'{block}.{q}'], want[q])
        print(f'{block} {q}: reference vs float64 restatement {e:.3e}, stored {dist:.3e}')
        assert dist < 2e-6, q                                        # fp32 rounding, nothing structural
        assert e <= dist * (1 + 1e-9) + 1e-12, q
    assert np.array_equal(fx[f'{block}.xs'] != 0, want['xs'] != 0) and np.array_equal(fx[f'{block}.a'] != 0, want['a'] != 0)
    assert ((fx[f'{block}.xs'] != 0).sum(1) == int(fx[f'{block}.top_m'])).all()
    assert ((fx[f'{block}.a'] != 0).sum(1) == int(fx[f'{block}.top_n'])).all()
    for g in ('x_tilde', 'a_tilde', 'eval_a_tilde', 'log_b'):
        assert float(fx[f'{block}.gap.{g}']) >= 1e-4, g


def _operator_input(n, C, seed):
    """n rows of C distinct multiples of 1/64 in [-1, 1] in random order; for n >= 5 rows 1..4 and the last row are
    replaced: values rounded to quarters (ties across every k boundary), zeros, alternating +-80, all +80, ties."""
    rng = np.random.RandomState(seed)
    grid = np.arange(-64, 65) / 64.
    S = np.stack([rng.permutation(grid)[:C] for _ in range(n)]).astype(np.float32)
    if n >= 5:
        S[1] = np.round(S[1] * 4) / 4
        S[2] = 0.
        S[3] = np.where(np.arange(C) % 2 == 0, 80., -80.)
        S[4] = 80.
        S[n - 1] = np.round(S[n - 1] * 2) / 2
    return S


def _row_err(got, ref):
    return np.abs(got - ref).max(-1) / np.abs(ref).max(-1)


def test_numpy_operator_mask_is_the_stable_top_k():
    for C in (1, 7, 20, 33, 64):
        S = _operator_input(257, C, seed=C)
        for k in sorted({1, max(C // 2, 1), C}):
            mask = ecf_restate.topk_mask(S, k)
            order = np.argsort(-S, axis=-1, kind='stable')[:, :k]
            want = np.zeros_like(mask)
            np.put_along_axis(want, order, True, axis=-1)
            assert np.array_equal(mask, want) and (mask.sum(-1) == k).all()
            for dtype in (np.float32, np.float64):
                A = ecf_restate.affiliation(S, k, 2., dtype)
                assert A.dtype == dtype and np.all(A[~mask] == 0) and np.all(A[mask] > 0)
    # the gradient restatement is the derivative of the operator with the mask held constant
    S = _operator_input(5, 7, seed=0).astype(np.float64)[:1]
    G = np.random.RandomState(1).randn(1, 7)
    St = torch.from_numpy(S).requires_grad_()
    (ecf_restate._affiliate(St, 3, .5) * torch.from_numpy(G)).sum().backward()
    assert np.allclose(ecf_restate.affiliation_backward(S, G, 3, .5), St.grad.numpy(), rtol=1e-12, atol=1e-14)


def test_several_processes_are_refused(tmp_path, monkeypatch):
    from hassaku_amd import experiment_helper
    from hassaku_amd.algorithms.algorithms_utils import AlgorithmsEnum
    from hassaku_amd.data.data_utils import DatasetsEnum
    monkeypatch.setattr(experiment_helper, 'maybe_init_distributed', lambda conf: 2)
    monkeypatch.setattr('torch.distributed.get_rank', lambda: 0)
    monkeypatch.setattr('torch.distributed.broadcast_object_list', lambda box, src=0: None)
    conf = {'data_path': str(tmp_path), 'model_save_path': str(tmp_path / 'm'),
            'running_settings': {'use_wandb': False}}
    with pytest.raises(ValueError, match='ecf runs in a single process'):
        experiment_helper.run_train_val(AlgorithmsEnum.ecf, DatasetsEnum.ml100k, conf)


# ------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize('C', (1, 7, 20, 33, 64))
@pytest.mark.parametrize('n', (1, 5, 257))
def test_affiliation_forward_and_backward(n, C):
    from hassaku_amd import hip_ops
    S = _operator_input(n, C, seed=100 * n + C)
    G = np.random.RandomState(n + C).randn(n, C).astype(np.float32)
    for k in sorted({1, max(C // 2, 1), C}):
        mask = ecf_restate.topk_mask(S, k)
        for t in (.5, 2.):
            outs = []
            for _ in range(2):
                Sd = torch.from_numpy(S).cuda().requires_grad_()
                A = hip_ops.ecf_affiliation(Sd, k, t)
                A.backward(torch.from_numpy(G).cuda())
                outs.append((A.detach().clone(), Sd.grad.clone()))
            assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])      # same bits
            A, dS = outs[0][0].cpu().numpy(), outs[0][1].cpu().numpy()
            assert A.shape == (n, C) and A.dtype == np.float32 and dS.shape == (n, C)
            assert np.array_equal(A != 0, mask) and np.all(A[~mask] == 0)
            for what, got, f64, f32 in (
                    ('A', A, ecf_restate.affiliation(S, k, t), ecf_restate.affiliation(S, k, t, np.float32)),
                    ('dS', dS, ecf_restate.affiliation_backward(S, G, k, t),
                     ecf_restate.affiliation_backward(S, G, k, t, np.float32))):
                assert f32.dtype == np.float32 and f64.dtype == np.float64
                err, bound = _row_err(got, f64), np.maximum(4 * _row_err(f32, f64), 1e-6)
                worst = int(np.argmax(err / bound))
                print(f'n {n} C {C} k {k} t {t} {what}: max row err {err.max():.3e}, worst err / bound '
                      f'{err[worst] / bound[worst]:.3f} (row {worst}, bound {bound[worst]:.3e})')
                assert np.all(err <= bound), what


@pytest.mark.gpu
def test_affiliation_refusals():
    from hassaku_amd import hip_ops
    assert hip_ops.ECF_MAX_CLUSTERS == 64
    S = torch.rand(6, 20, device='cuda')
    with pytest.raises(TypeError):
        hip_ops.ecf_affiliation(S.double(), 5, 2.)
    with pytest.raises(ValueError, match='contiguous'):
        hip_ops.ecf_affiliation(torch.rand(20, 6, device='cuda').T, 5, 2.)
    with pytest.raises(RuntimeError, match='no CPU path'):
        hip_ops.ecf_affiliation(S.cpu(), 5, 2.)
    with pytest.raises(ValueError, match='expected'):
        hip_ops.ecf_affiliation(S.reshape(2, 3, 20), 5, 2.)
    with pytest.raises(ValueError, match='65 clusters'):
        hip_ops.ecf_affiliation(torch.rand(3, 65, device='cuda'), 5, 2.)
    for k in (0, 21, 2.5, True):
        with pytest.raises(ValueError, match='top_k'):
            hip_ops.ecf_affiliation(S, k, 2.)
    for t in (0, -1., float('inf'), float('nan')):
        with pytest.raises(ValueError, match='temperature'):
            hip_ops.ecf_affiliation(S, 5, t)
    # the library's own checks, behind the Python ones
    from hassaku_amd import _lib
    lib = _lib.load()
    A = torch.empty_like(S)
    stream = torch.cuda.current_stream().cuda_stream
    for n, C, k, t in ((6, 65, 5, 2.), (6, 20, 0, 2.), (6, 20, 21, 2.), (6, 20, 5, 0.), (6, 20, 5, float('nan')),
                       (6, 20, 5, float('inf'))):
        assert lib.hsk_ecf_affiliation(S.data_ptr(), n, C, k, t, A.data_ptr(), stream) == 1        # HSK_ERR_INVALID
        assert lib.hsk_ecf_affiliation_backward(S.data_ptr(), S.data_ptr(), n, C, k, t, A.data_ptr(), stream) == 1
    empty = torch.empty(0, 20, device='cuda', requires_grad=True)
    out = hip_ops.ecf_affiliation(empty, 5, 2.)
    out.sum().backward()
    assert out.shape == (0, 20) and empty.grad.shape == (0, 20)


@pytest.mark.gpu
@pytest.mark.parametrize('block', BLOCKS)
def test_one_step_vs_golden(block):
    from hassaku_amd.train.rec_losses import RecBayesianPersonalizedRankingLoss
    fx = _gold()
    model = _gold_model(block, seed=5)
    model.load_state_dict(_init_state(block))
    model = model.to('cuda')
    assert model.x_indices.is_cuda and model.tag_weight.is_cuda
    u, i = torch.from_numpy(fx[f'{block}.u_idx']).cuda(), torch.from_numpy(fx[f'{block}.i_idx']).cuda()
    labels = torch.zeros(i.shape, device='cuda')
    labels[:, 0] = 1.
    scores = model(u, i)
    other = model.get_and_reset_other_loss()
    assert sorted(other) == ['cf_loss', 'ind_loss', 'reg_loss', 'ts_loss']
    (RecBayesianPersonalizedRankingLoss().compute_loss(scores, labels) + other['reg_loss']).backward()
    got = {'x_tilde': model._x_tildes, 'xs': model._xs, 'a': model.get_user_representations(u)[0], 'scores': scores,
           'cf_loss': other['cf_loss'], 'ind_loss': other['ind_loss'], 'ts_loss': other['ts_loss']}
    got.update({'grad.' + n: p.grad for n, p in model.named_parameters()})
    with torch.no_grad():
        i_repr = model.get_item_representations(torch.arange(model.n_items, device='cuda'))
        u_repr = model.get_user_representations(torch.from_numpy(fx['eval.u']).cuda())
        got['eval.scores'] = model.combine_user_item_representations(u_repr, i_repr)
    model.check_indices()
    got = {k: v.detach().cpu().numpy() for k, v in got.items()}
    assert sorted(got) == sorted(QUANTITIES)
    assert np.array_equal(got['xs'] != 0, fx[f'{block}.xs'] != 0)
    assert np.array_equal(got['a'] != 0, fx[f'{block}.a'] != 0)
    failed = []
    for q in QUANTITIES:
        e, bound = max_norm_err(got[q], fx[f'{block}.{q}']), max(4 * float(fx[f'{block}.dist.{q}']), 1e-5)
        print(f'{block} {q}: max_norm_err {e:.3e}, bound {bound:.3e}')
        if not e <= bound:
            failed.append(q)
    assert not failed
    assert torch.equal(other['reg_loss'], other['ts_loss'] + other['ind_loss'] + other['cf_loss'])    # the reference's order


@pytest.mark.gpu
def test_no_dense_matrix_on_the_device():
    from scipy import sparse as sp
    from hassaku_amd.algorithms.ecf_alg import ECF
    from hassaku_amd.data.csr import UserItemCsr
    from hassaku_amd.data.synthetic import generate_fast
    U, I, T, C = 4096, 8192, 512, 64
    d = generate_fast(U, I, 200000, seed=3)
    X = UserItemCsr.from_pairs(d.train[:, 0], d.train[:, 1], U, I)
    rng = np.random.RandomState(0)
    items, tags = np.repeat(np.arange(I), 3), rng.randint(0, T, 3 * I)
    inc = sp.csr_matrix((np.ones(3 * I), (items, tags)), shape=(I, T))
    inc.sum_duplicates()
    inc.data[:] = 1.
    weighted = inc @ sp.diags(np.log(I / (np.asarray(inc.sum(0)).ravel() + 1e-6)))
    torch.manual_seed(0)
    model = ECF(U, I, weighted, X, embedding_dim=32, n_clusters=C).to('cuda')
    u = torch.from_numpy(rng.randint(0, U, 256)).cuda()
    i = torch.from_numpy(rng.randint(0, I, (256, 5))).cuda()
    own = sum(t.numel() * t.element_size() for t in list(model.parameters()) + list(model.buffers()))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = model(u, i)
    (out.sum() + model.get_and_reset_other_loss()['reg_loss']).backward()
    torch.cuda.synchronize()
    peak, quarter = torch.cuda.max_memory_allocated() - before + own, U * I * 4 // 4
    print(f'model {own} bytes, forward + backward peak {peak} bytes with it; a quarter of the dense fp32 train matrix is '
          f'{quarter} bytes')
    assert peak < quarter
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    model.check_indices()


@pytest.mark.gpu
def test_run_train_val_test_through_the_plugin_surface(tmp_path, monkeypatch):
    """run_experiment's path: conf -> AlgorithmsEnum slot -> ECFTrainRecDataset -> Trainer (autograd path) -> full
    evaluation -> model.pth -> run_test on a model rebuilt from the train split.  max_patience must stay below n_epochs
    (conf_parser), so with n_epochs = 2 the second epoch runs only if the first improved on the initial model: one or two
    epochs are logged."""
    from hassaku_amd import experiment_helper
    from hassaku_amd.algorithms.algorithms_utils import AlgorithmsEnum
    from hassaku_amd.data.data_utils import DatasetsEnum
    from hassaku_amd.train import trainer as trainer_mod
    _write_dataset(str(tmp_path / 'data' / 'ml100k' / 'processed_dataset'))
    conf = {'data_path': str(tmp_path / 'data'), 'model_save_path': str(tmp_path / 'models'), 'embedding_dim': 16,
            'n_clusters': 24, 'top_n': 5, 'top_m': 5, 'top_p': 3, 'lr': 5e-3, 'wd': 1e-5, 'optimizer': 'adamw',
            'n_epochs': 2, 'max_patience': 1, 'train_batch_size': 128, 'neg_train': 4, 'rec_loss': 'bpr',
            'eval_batch_size': 64, 'device': 'cuda', 'running_settings': {'use_wandb': False, 'batch_verbose': False}}
    users = torch.tensor([0, 7, 33, 64, 299])
    seen = {'val': [], 'test': []}
    logs = []

    def recording(which, real):
        def run(alg, loader, evaluator, device='cpu', verbose=False):
            with torch.no_grad():
                i_repr = alg.get_item_representations(torch.arange(alg.n_items, device=device))
                s = alg.combine_user_item_representations(alg.get_user_representations(users.to(device)), i_repr)
            seen[which].append(s.cpu())
            return real(alg, loader, evaluator, device, verbose=verbose)
        return run

    monkeypatch.setattr(trainer_mod, 'evaluate_recommender_algorithm',
                        recording('val', trainer_mod.evaluate_recommender_algorithm))
    monkeypatch.setattr(experiment_helper, 'evaluate_recommender_algorithm',
                        recording('test', experiment_helper.evaluate_recommender_algorithm))
    real_log = trainer_mod.Trainer._log
    monkeypatch.setattr(trainer_mod.Trainer, '_log', lambda self, d: logs.append(dict(d)) or real_log(self, d))
    best, test, conf = experiment_helper.run_train_val_test(AlgorithmsEnum.ecf, DatasetsEnum.ml100k, conf)
    epochs = [d for d in logs if 'epoch_train_reg_loss' in d]
    assert len(epochs) in (1, 2)
    for d in epochs:
        assert all(np.isfinite(float(d[k])) for k in ('epoch_train_loss', 'epoch_train_rec_loss', 'epoch_train_reg_loss'))
        assert float(d['epoch_train_reg_loss']) > 0
    for metrics in (best, test):
        assert isinstance(metrics, dict) and 'ndcg@10' in metrics and any(k.startswith('group_1_') for k in metrics)
        for k, v in metrics.items():
            if '@' in k:
                assert np.isfinite(v) and 0 <= v <= 1, (k, v)
    path = os.path.join(conf['model_path'], 'model.pth')
    assert sorted(torch.load(path)) == sorted(KEYS)
    assert len(seen['val']) == len(epochs) + 1 and len(seen['test']) == 1          # before training and after each epoch
    saved = seen['val'][best['best_epoch'] + 1]
    assert saved.shape == (5, 200) and torch.equal(seen['test'][0], saved)
    assert not torch.equal(seen['val'][0], seen['val'][-1])          # training moved the scores
