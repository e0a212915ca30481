"""ALS: registry, conf, persistence and the numpy restatement (CPU); hsk_als_solve_f64, the model and the experiment
path against the restatement (GPU).

No reference golden can exist (the reference delegates ALS to the `implicit` package): the yardstick is numpy in fp64,
als_restate.py.  A solved row is held to 2 x row_bound (derived in als_restate.py's docstring: the conditioning of the
row's own system times the perturbations of forming it and of Cholesky; twice, because numpy's solve is one such
evaluation).  Every test that uses the bound prints the bound and the measured ratio first.

Inputs: g11 (300 x 200), islands (130 x 150, two disjoint communities, empty users and items, built as in
tests/test_svd.py) and s1500 (generate(3000, 1500, 150000, seed=3))."""
import ctypes
import functools
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import als_restate as ar
from conftest import REPO, load_golden

BAD_INDEX, NOT_SPD = 1, 8


@functools.lru_cache(maxsize=None)
def _input(name):
    """(train, val) CSRs of the input (val None where there is none)."""
    from hassaku_amd.data.csr import UserItemCsr
    if name == 'islands':
        rng = np.random.RandomState(1)
        X = rng.rand(130, 150) < 0.15
        X[:60, 70:] = False
        X[60:, :70] = False
        X[[0, 7, 129]] = False
        X[:, [3, 149]] = False
        rows, cols = np.nonzero(X)
        return UserItemCsr.from_pairs(rows, cols, 130, 150), None
    if name == 'g11':
        fx = load_golden('g11_knn_data.npz')
        n_users, n_items, tr, va = int(fx['n_users']), int(fx['n_items']), fx['train'], fx['val']
    else:
        from hassaku_amd.data.synthetic import generate
        d = generate(3000, 1500, 150000, seed=3)
        n_users, n_items, tr, va = d.n_users, d.n_items, d.train, d.val
    return (UserItemCsr.from_pairs(tr[:, 0], tr[:, 1], n_users, n_items),
            UserItemCsr.from_pairs(va[:, 0], va[:, 1], n_users, n_items))


def _csr(train):
    return np.asarray(train.indptr, np.int64), np.asarray(train.indices, np.int32)


# ------------------------------------------------------------------------------------------------------ CPU
def test_registry_resolves_als():
    from hassaku_amd.algorithms import algorithms_utils as au
    from hassaku_amd.algorithms.base_classes import FittedRecommenderAlgorithm
    from hassaku_amd.algorithms.mf_algs import AlternatingLeastSquare
    assert au.algorithm_by_name('als').value is AlternatingLeastSquare and au.algorithm_by_name('als').name == 'als'
    assert au.algorithm_by_name('als') is au.WeightedFactorAlgorithmsEnum.als
    assert au.OFFERED_ALGORITHM_NAMES == au.RUNNABLE_ALGORITHM_NAMES + ('als',)
    assert au.algorithm_by_name('mf') is au.AlgorithmsEnum.mf
    assert au.algorithm_by_name('svd') is au.FactorAlgorithmsEnum.svd
    assert issubclass(AlternatingLeastSquare, FittedRecommenderAlgorithm)
    with pytest.raises(KeyError):
        au.AlgorithmsEnum['als']
    with pytest.raises(KeyError):
        au.algorithm_by_name('rbmf')
    assert 'als' not in au.RUNNABLE_ALGORITHM_NAMES and au.WeightedFactorAlgorithmsEnum not in au._OTHER_FAMILIES


def test_cli_lists_als():
    """`--help` names als among the choices of -a (as a whole name in that list: the help text also holds the word
    "also"), and the list is OFFERED_ALGORITHM_NAMES."""
    import re
    from hassaku_amd.algorithms.algorithms_utils import OFFERED_ALGORITHM_NAMES
    out = subprocess.run([sys.executable, os.path.join(REPO, 'run_experiment.py'), '--help'], capture_output=True,
                         text=True, cwd=REPO, check=True).stdout
    listed = re.search(r'registry\s+name\s+of\s+the\s+model\s+\(([^)]*)\)', out)
    assert listed, out
    names = [n.strip() for n in listed.group(1).replace('\n', ' ').split(',')]
    assert 'als' in names and names == sorted(OFFERED_ALGORITHM_NAMES)


def test_cli_takes_als_and_resolves_it(tmp_path, capsys):
    """main() with -a als gets past the parser and the registry and as far as reading the conf file (which is not
    there); a name outside the registry (rbmf) is refused by the parser."""
    import run_experiment
    missing = str(tmp_path / 'no_such_conf.yml')
    with pytest.raises(AssertionError, match='not found'):
        run_experiment.main(['-a', 'als', '-d', 'ml100k', '-c', missing])
    assert 'Algorithm is als - Dataset is ml100k' in capsys.readouterr().out
    with pytest.raises(SystemExit) as refused:
        run_experiment.main(['-a', 'rbmf', '-c', missing])
    assert refused.value.code == 2 and 'invalid choice' in capsys.readouterr().err


GOOD_CONF = {'alpha': 40, 'factors': 16, 'regularization': 0.01, 'n_iterations': 3}


@pytest.mark.parametrize('change, msg', [
    ({'alpha': None}, 'needs alpha'), ({'factors': None}, 'needs factors'),
    ({'regularization': None}, 'needs regularization'), ({'n_iterations': None}, 'needs n_iterations'),
    ({'factors': 0}, r'in \[1, 128\]'), ({'factors': 129}, r'in \[1, 128\]'), ({'factors': 16.0}, 'must be an integer'),
    ({'factors': True}, 'must be an integer'), ({'factors': '16'}, 'must be an integer'),
    ({'n_iterations': 0}, '>= 1'), ({'n_iterations': 2.5}, 'must be an integer'),
    ({'n_iterations': True}, 'must be an integer'),
    ({'alpha': 0}, 'finite and > 0'), ({'alpha': -1.0}, 'finite and > 0'), ({'alpha': float('inf')}, 'finite and > 0'),
    ({'alpha': float('nan')}, 'finite and > 0'), ({'alpha': True}, 'must be a number'), ({'alpha': '40'}, 'must be a number'),
    ({'regularization': 0}, 'finite and > 0'), ({'regularization': 0.0}, 'finite and > 0'),
    ({'regularization': float('nan')}, 'finite and > 0'), ({'regularization': False}, 'must be a number'),
    ({'use_gpu': 1}, 'must be a bool'), ({'use_gpu': 'yes'}, 'must be a bool'),
])
def test_conf_validation(tmp_path, change, msg):
    from hassaku_amd.algorithms.algorithms_utils import algorithm_by_name
    from hassaku_amd.conf.conf_parser import parse_conf
    from hassaku_amd.data.data_utils import DatasetsEnum
    conf = dict(GOOD_CONF, data_path=str(tmp_path), model_save_path=str(tmp_path / 'm'))
    for key, value in change.items():
        if value is None:
            del conf[key]
        else:
            conf[key] = value
    with pytest.raises(ValueError, match=msg):
        parse_conf(conf, algorithm_by_name('als'), DatasetsEnum.ml1m)


def test_conf_builds_model_without_sgd_defaults(tmp_path):
    from hassaku_amd.algorithms.algorithms_utils import algorithm_by_name
    from hassaku_amd.algorithms.mf_algs import AlternatingLeastSquare
    from hassaku_amd.conf.conf_parser import parse_conf
    from hassaku_amd.data.data_utils import DatasetsEnum
    for extra in ({}, {'use_gpu': True}, {'use_gpu': False}):
        conf = parse_conf(dict(GOOD_CONF, data_path=str(tmp_path), model_save_path=str(tmp_path / 'm'), **extra),
                          algorithm_by_name('als'), DatasetsEnum.ml1m)
        assert conf['alg'] == 'als' and 'lr' not in conf and 'n_epochs' not in conf and 'optimizer' not in conf
        m = algorithm_by_name('als').value.build_from_conf(conf, None)
        assert isinstance(m, AlternatingLeastSquare) and m.name == 'AlternatingLeastSquare'
        assert (m.alpha, m.factors, m.regularization, m.n_iterations) == (40.0, 16, 0.01, 3)
    assert (AlternatingLeastSquare.SEED, ar.SEED) == (0, 0)
    u0, v0 = AlternatingLeastSquare.init_factors(7, 5, 3)
    assert np.array_equal(u0, ar.init(7, 5, 3)[0]) and np.array_equal(v0, ar.init(7, 5, 3)[1])
    assert u0.shape == (7, 3) and v0.shape == (5, 3) and 0 <= u0.min() and u0.max() < 0.01
    for bad in (dict(factors=129), dict(factors=0), dict(alpha=0), dict(regularization=0), dict(n_iterations=0),
                dict(use_gpu='yes'), dict(use_gpu=1)):
        with pytest.raises(ValueError):
            AlternatingLeastSquare(**dict(dict(alpha=1.0, factors=8, regularization=0.1, n_iterations=1), **bad))
    with pytest.raises(RuntimeError, match='fit'):
        m.score_rows(None)


def test_restated_half_sweep_is_the_textbook_form():
    """half_sweep against (Y^T C_r Y + reg I)^-1 Y^T C_r p_r with the dense diagonal C_r on a 30 x 20 matrix; rows
    without entries are exactly 0; the objective does not rise over a half-sweep."""
    rng = np.random.RandomState(5)
    X = (rng.rand(30, 20) < 0.2).astype(np.float64)
    X[[4, 17]] = 0
    ptr = np.concatenate([[0], np.cumsum(X.sum(1).astype(np.int64))])
    idx = np.nonzero(X)[1].astype(np.int32)
    assert np.array_equal(ar.dense((ptr, idx), 20), X)
    Y, k, alpha, reg = 0.3 * rng.standard_normal((20, 6)), 6, 7.0, 0.05
    got, bounds = ar.half_sweep((ptr, idx), Y, alpha, reg, with_bound=True)
    for r in range(30):
        C = np.diag(1.0 + (alpha - 1.0) * X[r])
        ref = np.linalg.solve(Y.T @ C @ Y + reg * np.eye(k), Y.T @ C @ X[r])
        if X[r].sum() == 0:
            assert np.all(got[r] == 0) and bounds[r] == 0
        else:
            err = np.linalg.norm(got[r] - ref) / np.linalg.norm(ref)
            assert err <= 2 * bounds[r] and 0 < bounds[r] < 1e-10
    t_ptr, t_idx = ar.transpose((ptr, idx), 20)
    assert np.array_equal(ar.dense((t_ptr, t_idx), 30), X.T)
    U0, V0 = ar.init(30, 20, k)
    U1 = ar.half_sweep((ptr, idx), V0, alpha, reg)
    V1 = ar.half_sweep((t_ptr, t_idx), U1, alpha, reg)
    o = [ar.objective(X, U0, V0, alpha, reg), ar.objective(X, U1, V0, alpha, reg), ar.objective(X, U1, V1, alpha, reg)]
    assert o[0] > o[1] > o[2]
    Uf, Vf = ar.fit((ptr, idx), 20, k, alpha, reg, 1)
    assert np.array_equal(Uf, U1) and np.array_equal(Vf, V1)


def test_model_npz_is_validated(tmp_path):
    """Files written with numpy alone: the reference's two keys load (float32: what `implicit` returns), shape, dtype
    and alg mismatches are refused, nothing is unpickled, more than 128 factors are refused."""
    from hassaku_amd.algorithms.mf_algs import AlternatingLeastSquare
    uf, vf = np.arange(12, dtype=np.float64).reshape(4, 3) / 7, np.arange(15, dtype=np.float64).reshape(5, 3) / 3
    path = os.path.join(tmp_path, 'model.npz')

    def fresh():
        return AlternatingLeastSquare(2.0, 9, 0.1, 1, device='cpu')
    np.savez(path, users_factors=uf.astype(np.float32), items_factors=vf.astype(np.float32))
    m = fresh()
    m.load_model_from_path(str(tmp_path))
    assert (m.n_users, m.n_items, m.factors) == (4, 5, 3)
    assert np.array_equal(m.users_factors.numpy(), uf.astype(np.float32).astype(np.float64))
    assert np.array_equal(m.items_factors.numpy(), vf.astype(np.float32).astype(np.float64))
    assert m.users_factors.stride(0) == 4 and m.users_factors.dtype.is_floating_point
    good = dict(users_factors=uf, items_factors=vf, alg=np.array('als'), alpha=np.float64(2.0), factors=np.int64(3),
                regularization=np.float64(0.1), n_iterations=np.int64(1))
    np.savez(path, **good)
    m.load_model_from_path(str(tmp_path))
    assert np.array_equal(m.users_factors.numpy(), uf)
    wide = np.ones((4, 129))
    for bad, msg in ((dict(alg=np.array('svd')), 'svd'), (dict(users_factors=uf[:, :2]), 'do not share'),
                     (dict(items_factors=vf[0]), '2-D float'), (dict(users_factors=uf.astype(np.int64)), '2-D float'),
                     (dict(users_factors=wide, items_factors=np.ones((5, 129))), r'in \[1, 128\]'),
                     (dict(factors=np.int64(4)), 'factors = 4'),
                     (dict(users_factors=np.array([[{}]], dtype=object)), 'object')):
        np.savez(path, **dict(good, **bad))
        f = fresh()
        with pytest.raises(ValueError, match=msg):
            f.load_model_from_path(str(tmp_path))
        assert f.items_factors is None
    np.savez(path, users_factors=uf)
    with pytest.raises(ValueError, match='no items_factors'):
        fresh().load_model_from_path(str(tmp_path))


# ------------------------------------------------------------------------------------------------------ GPU
DEGREES = (0, 1, 2, 31, 32, 33, 63, 64, 65, 200, 257)
N_COLS = 257
SOLVE_CASES = [(1, 40, 0.01), (2, 1, 0.01), (15, 0.5, 0.01), (16, 40, 1e-6), (17, 40, 0.01), (17, 1, 1e-6),
               (33, 0.5, 1e-6), (33, 40, 0.01), (64, 40, 0.01), (64, 1, 0.01), (65, 40, 1e-6), (96, 0.5, 0.01),
               (96, 40, 0.01), (127, 40, 1e-6), (128, 40, 0.01), (128, 1, 1e-6), (128, 0.5, 0.01)]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _block(a, extra=0, fill=np.nan):
    """a [n, b] on the device as the leading columns of a [n, round_up(b, 2) + extra] buffer filled with `fill`."""
    import torch
    n, b = a.shape
    buf = torch.full((n, b + (b & 1) + extra), fill, dtype=torch.float64, device='cuda')
    buf[:, :b] = torch.from_numpy(np.ascontiguousarray(a))
    return buf[:, :b]


@functools.lru_cache(maxsize=None)
def _solve_csr():
    """One row per degree of DEGREES over 257 columns, ids ascending."""
    rng = np.random.RandomState(11)
    rows = [np.sort(rng.choice(N_COLS, d, replace=False)).astype(np.int32) for d in DEGREES]
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64)
    return ptr, np.concatenate(rows).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _solve_y(k):
    return 0.3 * np.random.RandomState(100 + k).standard_normal((N_COLS, k))     # mixed signs


def _solve(csr, Y, alpha, reg, G=None, order=None, status=None):
    from hassaku_amd import hip_ops
    ptr, idx = csr
    dY = _block(Y, extra=2)
    dG = hip_ops.svd_gram(dY) if G is None else _dev(G)
    out = _block(np.full((len(ptr) - 1, Y.shape[1]), np.nan), extra=2)
    res = hip_ops.als_solve((_dev(ptr), _dev(idx), Y.shape[0]), dY, dG, alpha, reg,
                            order=None if order is None else _dev(np.asarray(order, np.int32)), out=out, status=status)
    assert res.data_ptr() == out.data_ptr()
    return res.cpu().numpy(), out


def _assert_rows_within_bound(what, got, ref, bounds):
    errs = ar.row_errors(got, ref)
    some = bounds > 0
    ratio = float((errs[some] / (2 * bounds[some])).max()) if some.any() else 0.0
    print(f'{what}: row_bound from {bounds[some].min():.3e} to {bounds[some].max():.3e}; worst row at {ratio:.3e} of '
          f'2 x its bound')
    assert np.all(got[~some] == 0) and not np.signbit(got[~some]).any()
    assert np.isfinite(bounds).all() and ratio <= 1


@pytest.mark.gpu
@pytest.mark.parametrize('k, alpha, reg', SOLVE_CASES)
def test_solve_against_numpy(k, alpha, reg):
    """hsk_als_solve_f64 row by row against numpy.linalg.solve within 2 x row_bound; the degree-0 row exactly 0; the
    padding of the output untouched; the status word clear."""
    import torch
    csr, Y = _solve_csr(), _solve_y(k)
    ref, bounds = ar.half_sweep(csr, Y, alpha, reg, with_bound=True)
    status = torch.zeros(1, dtype=torch.int32, device='cuda')
    got, out = _solve(csr, Y, alpha, reg, status=status)
    assert got.shape == (len(DEGREES), k) and not np.isnan(got).any()
    _assert_rows_within_bound(f'solve k {k} alpha {alpha} reg {reg}', got, ref, bounds)
    assert np.all(got[0] == 0) and bounds[0] == 0
    whole = torch.as_strided(out, (len(DEGREES), out.stride(0)), (out.stride(0), 1)).cpu().numpy()
    assert np.isnan(whole[:, k:]).all()
    assert int(status.item()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize('k', [17, 128])
def test_solve_is_deterministic(k):
    """Two calls, a call with `order` reversed and one with the longest rows first, and every row solved alone in a
    one-row CSR: all bit for bit the same."""
    csr, Y = _solve_csr(), _solve_y(k)
    ptr, idx = csr
    G = Y.T @ Y
    n = len(DEGREES)
    first, _ = _solve(csr, Y, 40.0, 0.01, G=G)
    assert np.array_equal(_solve(csr, Y, 40.0, 0.01, G=G)[0], first)
    assert np.array_equal(_solve(csr, Y, 40.0, 0.01, G=G, order=np.arange(n)[::-1])[0], first)
    assert np.array_equal(_solve(csr, Y, 40.0, 0.01, G=G, order=np.argsort(-np.diff(ptr), kind='stable'))[0], first)
    for r in range(n):
        one = (np.array([0, ptr[r + 1] - ptr[r]], np.int64), idx[ptr[r]:ptr[r + 1]] if ptr[r + 1] > ptr[r]
               else np.zeros(1, np.int32))
        assert np.array_equal(_solve(one, Y, 40.0, 0.01, G=G)[0][0], first[r]), f'row {r} alone'


@pytest.mark.gpu
def test_solve_refusals_and_status():
    """k = 0, k = 129, an odd ldy, alpha = 0, reg = 0 and NaN: HSK_ERR_INVALID from the library.  A column id of -1 or
    n_cols: HSK_STATUS_BAD_INDEX, the row as without that entry.  One inf in Y: HSK_STATUS_NOT_SPD and a zero row for
    the rows that touch it, the others as they were."""
    import torch
    from hassaku_amd import _lib, hip_ops
    lib = _lib.load()
    k = 17
    csr, Y = _solve_csr(), _solve_y(k)
    ptr, idx = csr
    G = Y.T @ Y
    dptr, didx, dY, dG = _dev(ptr), _dev(idx), _block(Y), _dev(G)
    out = _block(np.zeros((len(DEGREES), k)))
    status = torch.zeros(1, dtype=torch.int32, device='cuda')
    nan = float('nan')

    def call(k_=k, ldy=dY.stride(0), alpha=40.0, reg=0.01):
        return lib.hsk_als_solve_f64(dptr.data_ptr(), didx.data_ptr(), len(DEGREES), N_COLS, None, dY.data_ptr(), ldy,
                                     k_, dG.data_ptr(), k, alpha, reg, out.data_ptr(), out.stride(0),
                                     status.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert dY.stride(0) == 18
    for kw in (dict(k_=0), dict(k_=129), dict(ldy=17), dict(ldy=19), dict(alpha=0.0), dict(reg=0.0), dict(alpha=nan),
               dict(reg=nan), dict(alpha=float('inf')), dict(alpha=-1.0), dict(reg=-0.01)):
        assert call(**kw) == 1, kw          # HSK_ERR_INVALID
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and np.all(out.cpu().numpy() == 0)   # the refused calls launched nothing
    assert call() == 0
    assert int(status.item()) == 0 and np.any(out.cpu().numpy() != 0)
    with pytest.raises(RuntimeError, match=r'code 1.*k 129 outside \[1, 128\]'):
        wide = torch.zeros((N_COLS, 130), dtype=torch.float64, device='cuda')[:, :129]
        hip_ops.als_solve((dptr, didx, N_COLS), wide, torch.zeros((129, 129), dtype=torch.float64, device='cuda'), 2.0, 0.1)
    assert hip_ops.ALS_MAX_FACTORS == 128

    ref, bounds = ar.half_sweep(csr, Y, 40.0, 0.01, with_bound=True)
    clean, _ = _solve(csr, Y, 40.0, 0.01, G=G)
    # Appended bad ids are held bit for bit: row 5 (33 ids) with n_cols in a slot of its last block that read as zero
    # before, row 7 (64 ids) with -1 opening a third block that holds nothing but zeros -- every sum sees the terms it
    # saw without the entry, in the same places, plus exact zeros.  Row 3 (31 ids) has -1 in FRONT: b_r is still the
    # same bits (0.0 + y_1 + ...), but every entry moves one slot, so the products y y^T fall into other groups of
    # four inside v_mfma_f64_16x16x4_f64 ((0, y1, y2, y3) (y4 ...) instead of (y1, y2, y3, y4) ...) and fp64 addition
    # does not associate: bit-equality is not guaranteed there, and the row is held to its bound instead.
    rows = [idx[ptr[r]:ptr[r + 1]] for r in range(len(DEGREES))]
    rows[5] = np.concatenate([rows[5], [N_COLS]]).astype(np.int32)
    rows[7] = np.concatenate([rows[7], [-1]]).astype(np.int32)
    rows[3] = np.concatenate([[-1], rows[3]]).astype(np.int32)
    bad = (np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64), np.concatenate(rows))
    status.zero_()
    got, _ = _solve(bad, Y, 40.0, 0.01, G=G, status=status)
    assert int(status.item()) == BAD_INDEX
    _assert_rows_within_bound('rows with bad ids', got, ref, bounds)
    keep = np.arange(len(DEGREES)) != 3
    assert np.array_equal(got[keep], clean[keep])

    Yi = Y.copy()
    hit = int(rows[4][7])                      # an id of row 4 (32 ids)
    Yi[hit, 3] = np.inf
    touched = np.array([hit in set(x.tolist()) for x in rows])
    assert touched[4] and touched[10] and not touched[0] and not touched.all()
    for alpha in (40.0, 1.0):
        status.zero_()
        got, _ = _solve(csr, Yi, alpha, 0.01, G=G, status=status)       # G of the finite Y: only the row's own sums blow up
        assert int(status.item()) == NOT_SPD
        assert np.all(got[touched] == 0) and np.isfinite(got).all()
        assert np.array_equal(got[~touched], _solve(csr, Y, alpha, 0.01, G=G)[0][~touched])
    torch.cuda.synchronize()


def _fit(name, k, alpha, reg, n_iterations):
    from hassaku_amd.algorithms.mf_algs import AlternatingLeastSquare
    m = AlternatingLeastSquare(alpha, k, reg, n_iterations)
    m.fit(_input(name)[0])
    return m


@pytest.mark.gpu
@pytest.mark.parametrize('name, k, alpha, reg', [('g11', 64, 40.0, 0.01), ('islands', 33, 40.0, 0.01),
                                                 ('islands', 128, 0.5, 0.01), ('s1500', 17, 40.0, 0.01)])
def test_fit_one_iteration(name, k, alpha, reg):
    """users_factors against half_sweep(X, the start's items), items_factors against half_sweep(X^T, the device's
    users_factors), each row within 2 x row_bound; users and items without entries exactly 0.  (islands at k = 128 has
    more factors than users with entries, so the items' G = U^T U is singular and A_r rests on reg alone: at
    reg = 1e-6 kappa_2 eps >= 1 in the restatement itself and the bound says nothing, so that case is run at
    reg = 0.01, where the largest item bound is 1.4e-7.)"""
    train = _input(name)[0]
    csr = _csr(train)
    m = _fit(name, k, alpha, reg, 1)
    Uf, Vf = m.users_factors.cpu().numpy(), m.items_factors.cpu().numpy()
    assert Uf.shape == (train.n_rows, k) and Vf.shape == (train.n_cols, k)
    assert (m.n_users, m.n_items) == (train.n_rows, train.n_cols)
    _, V0 = ar.init(train.n_rows, train.n_cols, k)
    ref_u, bound_u = ar.half_sweep(csr, V0, alpha, reg, with_bound=True)
    _assert_rows_within_bound(f'{name} k {k} users', Uf, ref_u, bound_u)
    ref_v, bound_v = ar.half_sweep(ar.transpose(csr, train.n_cols), Uf, alpha, reg, with_bound=True)
    _assert_rows_within_bound(f'{name} k {k} items', Vf, ref_v, bound_v)
    empty_u, empty_v = np.diff(csr[0]) == 0, np.bincount(csr[1], minlength=train.n_cols) == 0
    if name == 'islands':
        assert empty_u.sum() >= 3 and empty_v.sum() >= 2
    assert np.all(Uf[empty_u] == 0) and np.all(Vf[empty_v] == 0)
    assert np.array_equal(bound_u == 0, empty_u) and np.array_equal(bound_v == 0, empty_v)


@pytest.mark.gpu
@pytest.mark.parametrize('k, alpha, reg', [(8, 1.0, 0.01), (17, 0.5, 0.01), (64, 40.0, 0.01), (128, 40.0, 0.01),
                                           (128, 40.0, 1e-6), (100, 1.0, 1e-6)])
def test_fit_four_iterations(k, alpha, reg):
    """On g11: the last half-sweep is consistent (the items recomputed in numpy from the device's users, within the
    bound), and the fits with 1 .. 4 iterations from the same start give objective(U_t, V_t-1), objective(U_t, V_t),
    computed in numpy with V_0 from init: strictly decreasing at every half-sweep (the restatement loses at least
    0.4 % at each for these six cases, so no slack is given)."""
    train = _input('g11')[0]
    csr = _csr(train)
    X = ar.dense(csr, train.n_cols)
    fits = [_fit('g11', k, alpha, reg, t) for t in (1, 2, 3, 4)]
    Us = [m.users_factors.cpu().numpy() for m in fits]
    Vs = [ar.init(train.n_rows, train.n_cols, k)[1]] + [m.items_factors.cpu().numpy() for m in fits]
    ref_v, bound_v = ar.half_sweep(ar.transpose(csr, train.n_cols), Us[3], alpha, reg, with_bound=True)
    _assert_rows_within_bound(f'g11 k {k} alpha {alpha} reg {reg}: items of iteration 4', Vs[4], ref_v, bound_v)
    seq = []
    for t in range(4):
        seq += [ar.objective(X, Us[t], Vs[t], alpha, reg), ar.objective(X, Us[t], Vs[t + 1], alpha, reg)]
    print(f'g11 k {k} alpha {alpha} reg {reg}: objective ' + ' '.join(f'{o:.9e}' for o in seq))
    assert np.isfinite(seq).all() and all(b < a for a, b in zip(seq, seq[1:]))


@pytest.mark.gpu
def test_scoring_evaluation_and_reload(tmp_path):
    """score_rows against U V^T from the device's own factors within 2 gamma_{k+1} sum |u| |v|; excluded columns -inf;
    an out-of-range user raises through check_indices; evaluate_recommender_algorithm returns the usual keys; a model
    saved and loaded gives bitwise the same rows."""
    import torch
    from hassaku_amd.algorithms.mf_algs import AlternatingLeastSquare
    from hassaku_amd.eval.eval import FullEvaluator, evaluate_recommender_algorithm
    train, val = _input('g11')
    k = 17
    m = _fit('g11', k, 40.0, 0.01, 2)
    Uf, Vf = m.users_factors.cpu().numpy(), m.items_factors.cpu().numpy()
    users = np.concatenate([np.arange(train.n_rows), [3, 3, 0]]).astype(np.int64)
    got = m.score_rows(_dev(users)).cpu().numpy()
    bound = 2 * ar.gamma(k + 1) * (np.abs(Uf[users]) @ np.abs(Vf).T)
    worst = float((np.abs(got - Uf[users] @ Vf.T) / bound).max())
    print(f'score_rows k {k}: at most {worst:.3e} of 2 gamma_(k+1) sum |u_f| |v_f|')
    assert got.shape == (len(users), train.n_cols) and worst <= 1
    ep, ei = train.to_device('cuda')
    masked = got.copy()
    for q, u in enumerate(users):
        masked[q, train.row(int(u))] = -np.inf
    got_x = m.score_rows(_dev(users), excl=(ep, ei)).cpu().numpy()
    assert np.array_equal(got_x, masked)
    m.check_indices()
    m.score_rows(_dev(np.array([1, train.n_rows], dtype=np.int64)))
    with pytest.raises(IndexError):
        m.check_indices()
    m.check_indices()
    lp, li = val.to_device('cuda')
    dataset = types.SimpleNamespace(n_users=train.n_rows, n_items=train.n_cols, device_arrays=lambda device: {
        'label_indptr': lp, 'label_indices': li, 'excl_indptr': ep, 'excl_indices': ei})
    res = evaluate_recommender_algorithm(m, types.SimpleNamespace(dataset=dataset), FullEvaluator(False, 0))
    for key in (f'{name}@{n}' for name in ('precision', 'recall', 'ndcg') for n in (5, 10, 50, 100)):
        assert key in res, (key, sorted(res))
    assert 0 < float(np.mean(res['ndcg@10'])) <= 1
    m.save_model_to_path(str(tmp_path))
    with np.load(os.path.join(tmp_path, 'model.npz'), allow_pickle=False) as f:
        assert set(f.files) == {'users_factors', 'items_factors', 'alg', 'alpha', 'factors', 'regularization',
                                'n_iterations'}
        assert str(f['alg']) == 'als' and int(f['factors']) == k and float(f['alpha']) == 40.0
        assert f['users_factors'].dtype == np.float64 and np.array_equal(f['users_factors'], Uf)
    m2 = AlternatingLeastSquare(1.0, 5, 1.0, 1)
    m2.load_model_from_path(str(tmp_path))
    assert m2.factors == k
    assert np.array_equal(m2.score_rows(_dev(users)).cpu().numpy(), got)
    assert np.array_equal(m2.score_rows(_dev(users), excl=(ep, ei)).cpu().numpy(), got_x)
    m2.check_indices()
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_fit_failure_modes(monkeypatch):
    """A fit refused for lack of device memory, and a fit whose solver raises a status bit, leave no model; more than
    128 factors are refused before anything is allocated."""
    import torch
    from hassaku_amd import hip_ops
    from hassaku_amd.algorithms.mf_algs import AlternatingLeastSquare
    train = _input('islands')[0]
    with pytest.raises(ValueError, match=r'in \[1, 128\]'):
        AlternatingLeastSquare(40.0, 129, 0.01, 1)
    m = AlternatingLeastSquare(40.0, 8, 0.01, 1)
    m.fit(train)
    assert m.items_factors is not None
    nnz = int(train.nnz)
    need = m.fit_bytes(130, 150, nnz)
    assert need == ((130 + 150) * (8 * 8 + 4) + max(hip_ops.svd_gram_ws_bytes(130, 8), hip_ops.svd_gram_ws_bytes(150, 8))
                    + 8 * 8 * 8 + (131 + 151) * 8 + 2 * nnz * 4 + 5 * nnz * 8 + 150 * 8)
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, 'mem_get_info', lambda device=None: (need - 1, 1 << 40))
        with pytest.raises(ValueError, match='needs .* bytes of device memory, .* are free'):
            m.fit(train)
    assert m.items_factors is None and m.users_factors is None
    with pytest.raises(RuntimeError, match='fit'):
        m.score_rows(_dev(np.array([0], dtype=np.int64)))
    m.fit(train)
    assert m.items_factors is not None
    real = hip_ops.als_solve

    def raising(*args, **kw):            # a solver that reports a failed pivot
        kw['status'].fill_(NOT_SPD)
        return real(*args, **kw)
    with monkeypatch.context() as mp:
        mp.setattr(hip_ops, 'als_solve', raising)
        with pytest.raises(ValueError, match='HSK_STATUS_NOT_SPD'):
            m.fit(train)
    assert m.items_factors is None and m.users_factors is None


@pytest.mark.gpu
def test_run_train_val_test(tmp_path):
    """run_experiment's path with -a als on the toy dataset: conf -> slot -> fit -> val metrics -> model.npz -> test
    metrics through load_model_from_path; the saved factors are the deterministic fit's."""
    from hassaku_amd.algorithms.algorithms_utils import algorithm_by_name
    from hassaku_amd.algorithms.mf_algs import AlternatingLeastSquare
    from hassaku_amd.data.csr import UserItemCsr
    from hassaku_amd.data.data_utils import DatasetsEnum
    from hassaku_amd.data.synthetic import generate, write_csv_dataset
    from hassaku_amd.experiment_helper import run_train_val_test
    d = generate(250, 180, 6000, seed=7, n_groups=2)
    write_csv_dataset(d, str(tmp_path / 'data' / 'ml100k' / 'processed_dataset'))
    conf = {'data_path': str(tmp_path / 'data'), 'model_save_path': str(tmp_path / 'models'), 'alpha': 40,
            'factors': 12, 'regularization': 0.01, 'n_iterations': 3, 'use_gpu': True, 'eval_batch_size': 64,
            'running_settings': {'use_wandb': False, 'batch_verbose': False}}
    best, test, conf = run_train_val_test(algorithm_by_name('als'), DatasetsEnum.ml100k, conf)
    assert len(test) == 36 and 0 < test['ndcg@10'] <= 1 and 0 < best['ndcg@10'] <= 1
    path = os.path.join(conf['model_path'], 'model.npz')
    with np.load(path, allow_pickle=False) as f:
        uf, vf = f['users_factors'], f['items_factors']
        assert uf.dtype == vf.dtype == np.float64 and uf.shape == (250, 12) and vf.shape == (180, 12)
        assert str(f['alg']) == 'als' and int(f['n_iterations']) == 3
    train = UserItemCsr.from_pairs(d.train[:, 0], d.train[:, 1], d.n_users, d.n_items)
    m = AlternatingLeastSquare(40, 12, 0.01, 3)
    m.fit(train)
    assert np.array_equal(m.items_factors.cpu().numpy(), vf) and np.array_equal(m.users_factors.cpu().numpy(), uf)
    csr = _csr(train)
    ref_v, bound_v = ar.half_sweep(ar.transpose(csr, d.n_items), uf, 40.0, 0.01, with_bound=True)
    _assert_rows_within_bound('toy dataset: items of iteration 3', vf, ref_v, bound_v)
    # the same run from the command line: run_experiment.py -a als trains, validates, saves and tests
    import glob
    import yaml
    import run_experiment
    cli_conf = {'data_path': str(tmp_path / 'data'), 'model_save_path': str(tmp_path / 'cli_models'), 'alpha': 40,
                'factors': 12, 'regularization': 0.01, 'n_iterations': 3, 'eval_batch_size': 64,
                'running_settings': {'use_wandb': False, 'batch_verbose': False}}
    with open(tmp_path / 'conf.yml', 'w') as fh:
        yaml.dump(cli_conf, fh)
    assert run_experiment.main(['-a', 'als', '-d', 'ml100k', '-c', str(tmp_path / 'conf.yml')]) == 0
    saved = glob.glob(str(tmp_path / 'cli_models' / 'als-ml100k' / 'single_runs' / '*' / 'model.npz'))
    assert len(saved) == 1
    with np.load(saved[0], allow_pickle=False) as f:
        assert np.array_equal(f['users_factors'], uf) and np.array_equal(f['items_factors'], vf)
