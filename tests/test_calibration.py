"""Calibration metrics (FullEvaluatorCalibrationDecorator): the torch distance functions, the CPU decorator and the two
matrix builders against the reference's g16 golden (CPU); hsk_calibration_metrics against the numpy restatement
(tests/calibration_restate.py) and the golden, and the decorated evaluation paths end to end (GPU).

Bounds.  Kernel and restatement compute the same fp64 expressions on the same inputs -- the item rows are added in
the same order, so q is the same number on both sides -- and differ by the ulp or two of log / sqrt and by the order
in which the bins are added up.  A finite result is therefore held to |dev - restate| <= C 2^-52 S on hellinger^2, js^2
and kl, S the scale the restatement returns (the sum of the magnitudes that were added); non-finite results must agree
in kind and position.  C = 4 x the worst ratio seen over the whole shape list on an MI355X (MEASUREMENTS.md,
"Calibration metrics"); every such test prints its worst ratio first.

The reference computes in float32; what that costs was measured by the generator on the fixture itself (reference
against restatement, fp32_err_* of the npz) and four times that is the bound of anything held to the golden.  A
jensen-shannon row whose fp64 js^2 is below 1e-6 is compared on js^2 only."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import calibration_restate as cr
from conftest import REPO, load_golden

ULP = 2.0 ** -52
C_KERNEL = 4 * 15.54         # the worst ratio was 15.54 (3 bins, float32 items); anything near 2^10 would not be rounding
KS = [100, 50, 10, 5]
PREFIXES = ('tag', 'pop')
KINDS = cr.NAMES
BETAS = (('b0p01', .01), ('b0', 0.))
JS2_SMALL = 1e-6
PAD = 0x7fffffff


@functools.lru_cache(maxsize=None)
def _gold():
    return load_golden('g16_calibration.npz')


def _mats(g, prefix):
    """(user_mtx, item_mtx) float32 torch tensors of a prefix"""
    import torch
    return torch.from_numpy(g[f'user_{prefix}']), torch.from_numpy(g[f'item_{prefix}'])


def _nested(base, g, beta=.01, kw=None):
    from hassaku_amd.eval.eval import FullEvaluatorCalibrationDecorator
    ev = base
    for prefix in PREFIXES:
        user_mtx, item_mtx = _mats(g, prefix)
        ev = FullEvaluatorCalibrationDecorator(ev, item_mtx, user_mtx, metric_name_prefix=prefix,
                                               beta_smoothening=beta, **(kw or {}))
    return ev


def _ranking_logits(top_ids, n_items):
    """float32 logits whose top-k are exactly top_ids, in order"""
    import torch
    R, k = top_ids.shape
    logits = torch.full((R, n_items), -1., dtype=torch.float32)
    logits.scatter_(1, torch.from_numpy(top_ids.astype(np.int64)),
                    torch.arange(k, 0, -1, dtype=torch.float32).expand(R, k).contiguous())
    return logits


def _write_g11(folder, g, drop_user=None):
    """the g11 dataset with the fixture's tag files under folder/processed_dataset"""
    import pandas as pd
    from hassaku_amd.data.synthetic import generate, write_csv_dataset
    d = generate(300, 200, 6000, seed=11, n_groups=2)
    assert np.array_equal(d.train, load_golden('g11_knn_data.npz')['train'])
    path = os.path.join(str(folder), 'processed_dataset')
    write_csv_dataset(d, path)
    if drop_user is not None:
        keep = d.train[d.train[:, 0] != drop_user]
        pd.DataFrame({'user_idx': keep[:, 0], 'item_idx': keep[:, 1]}).to_csv(
            os.path.join(path, 'listening_history_train.csv'), index=False)
    pd.DataFrame({'tag_idx': np.arange(int(g['n_tags']))}).to_csv(os.path.join(path, 'tag_idxs.csv'), index=False)
    pd.DataFrame({'item_idx': g['item_tags'][:, 0], 'tag_idx': g['item_tags'][:, 1]}).to_csv(
        os.path.join(path, 'item_tag_idxs.csv'), index=False)
    return d, path


def _same_non_finite(got, ref, what=''):
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f'{what}: NaN positions differ'
    assert np.array_equal(np.isposinf(got), np.isposinf(ref)), f'{what}: +inf positions differ'
    assert np.array_equal(np.isneginf(got), np.isneginf(ref)), f'{what}: -inf positions differ'


def _hold_to_golden(got, g, tag, what):
    """got: name -> [48] per-user values; held to the golden's columns within 4 x the measured float32 cost"""
    beta = dict(BETAS)[tag]
    names = [str(n) for n in g['names']]
    worst = np.zeros((2, 4))
    for pi, prefix in enumerate(PREFIXES):
        rs = cr.calibration(g['top_ids'], g['users'], g[f'item_{prefix}'], g[f'user_{prefix}'], beta, KS)
        for t, k in enumerate(KS):
            for j, kind in enumerate(KINDS):
                name = f'{prefix}_{kind}@{k}'
                ref = g[f'per_user_{tag}'][:, names.index(name)].astype(np.float64)
                val = np.asarray(got[name], np.float64)
                _same_non_finite(val, ref, f'{what} {name}')
                fin = np.isfinite(ref)
                if kind == 'jensen_shannon_distance':
                    small = fin & (rs['compared'][:, t, j] < JS2_SMALL)
                    fin &= ~small
                    if small.any():
                        worst[pi, 3] = max(worst[pi, 3], np.abs(val[small] ** 2 - ref[small] ** 2).max())
                if fin.any():
                    worst[pi, j] = max(worst[pi, j], np.abs(val[fin] - ref[fin]).max())
    bound = 4 * g[f'fp32_err_{tag}']
    print(f'{what} {tag}: worst |got - golden| [prefix, (hel, js, kl, js2 small)]\n{worst}\nbound\n{bound}')
    assert (worst <= bound).all()


# ------------------------------------------------------------------------------------------------------ CPU
def test_restatement_reproduces_the_golden():
    """The yardstick itself: the fp64 restatement against the reference's float32 run, with the generator's figures."""
    g = _gold()
    for tag, beta in BETAS:
        got = {}
        for prefix in PREFIXES:
            got.update(cr.metric_dict(g['top_ids'], g['users'], g[f'item_{prefix}'], g[f'user_{prefix}'], beta, KS, prefix))
        _hold_to_golden(got, g, tag, 'restatement')
    assert not np.isfinite(g['per_user_b0']).all() and np.isfinite(g['per_user_b0p01']).all()


def test_distance_functions():
    import torch
    from hassaku_amd.eval.metrics import hellinger_distance, jensen_shannon_distance, kl_divergence
    g = _gold()
    fns = dict(zip(KINDS, (hellinger_distance, jensen_shannon_distance, kl_divergence)))
    users, ids = torch.from_numpy(g['users']), torch.from_numpy(g['top_ids'].astype(np.int64))
    for tag, beta in BETAS:
        got = {}
        for prefix in PREFIXES:
            user_mtx, item_mtx = _mats(g, prefix)
            p = user_mtx[users]
            for k in KS:
                q = beta * p + (1 - beta) * (item_mtx[ids[:, :k]].sum(1) / k)
                for kind, fn in fns.items():
                    out = fn(p, q)
                    assert out.shape == (len(users),) and out.dtype == torch.float32
                    got[f'{prefix}_{kind}@{k}'] = out.numpy()
        _hold_to_golden(got, g, tag, 'torch functions')
    # closed forms, fp64: p = (.5, .5), q = (.25, .75); batched leading axes; the IEEE outcomes of an empty bin
    p, q = torch.tensor([.5, .5], dtype=torch.float64), torch.tensor([.25, .75], dtype=torch.float64)
    assert abs(float(kl_divergence(p, q)) - .5 * np.log(4 / 3)) < 1e-15
    assert abs(float(hellinger_distance(p, q)) - np.sqrt(1 - (np.sqrt(.125) + np.sqrt(.375)))) < 1e-15
    assert float(jensen_shannon_distance(p, q)) == float(jensen_shannon_distance(q, p)) > 0
    assert float(hellinger_distance(p, p)) == 0 and float(kl_divergence(q, q)) == 0 and float(jensen_shannon_distance(q, q)) == 0
    assert hellinger_distance(torch.rand(2, 3, 7), torch.rand(2, 3, 7)).shape == (2, 3)
    e = torch.tensor([1., 0.])
    assert float(kl_divergence(p.float(), e)) == np.inf and np.isnan(float(kl_divergence(e, p.float())))
    assert np.isnan(float(jensen_shannon_distance(p.float(), e))) and float(hellinger_distance(e, e)) == 0


@pytest.mark.parametrize('tag', [t for t, _ in BETAS])
def test_cpu_decorator_per_user(tag):
    import torch
    from hassaku_amd.eval.eval import FullEvaluator
    g = _gold()
    ev = _nested(FullEvaluator(aggr_by_group=False), g, dict(BETAS)[tag])
    users = torch.from_numpy(g['users'])
    ev.eval_batch(users, _ranking_logits(g['top_ids'], g['labels'].shape[1]), torch.from_numpy(g['labels'].astype(np.float32)))
    res = ev.get_results()
    assert len(res) == 12 + 2 * 12 and set(str(n) for n in g['names']) <= set(res)
    _hold_to_golden(res, g, tag, 'cpu decorator (eval_batch)')
    # the ranked entry gives the same numbers and leaves the base metrics alone
    ev.eval_topk(users, torch.from_numpy(g['top_ids']))
    res2 = ev.get_results()
    assert len(res2) == 24 and all(np.array_equal(res2[n], res[n], equal_nan=True) for n in res2)


def test_cpu_decorator_aggregated_two_groups():
    """The aggregated dictionary with both groups: a mean of 48 (or a group's share of them) per-user values.  On top of
    the per-user bound the reference adds them up in float32: n 2^-24 of the mean."""
    import torch
    from hassaku_amd.eval.eval import FullEvaluator
    g = _gold()
    ev = _nested(FullEvaluator(aggr_by_group=True, n_groups=2, user_to_user_group=torch.from_numpy(g['user_group'])), g)
    users = torch.from_numpy(g['users'])
    half = len(users) // 2                      # two batches: the sums carry over
    logits, labels = _ranking_logits(g['top_ids'], g['labels'].shape[1]), torch.from_numpy(g['labels'].astype(np.float32))
    ev.eval_batch(users[:half], logits[:half], labels[:half])
    ev.eval_batch(users[half:], logits[half:], labels[half:])
    res = ev.get_results()
    ref = dict(zip((str(n) for n in g['aggr_names']), g['aggr_values']))
    assert set(res) == set(ref) and len(ref) == 3 * 36
    bound4 = 4 * g['fp32_err_b0p01']
    for name, want in ref.items():
        kind = next((j for j, kd in enumerate(KINDS) if f'_{kd}@' in name), None)
        if kind is None:
            assert abs(res[name] - want) <= 1e-6, name          # precision / recall / ndcg, as in the other suites
            continue
        prefix = PREFIXES.index(name.replace('group_0_', '').replace('group_1_', '').split('_')[0])
        assert np.isfinite(want) and abs(res[name] - want) <= bound4[prefix, kind] + len(users) * 2.0 ** -24 * abs(want), name
    assert ev.get_results() == {}               # reset through the decorators


def test_builders_match_the_golden(tmp_path):
    import torch
    from hassaku_amd.data.data_utils import build_user_and_item_pop_matrix, build_user_and_item_tag_matrix
    g = _gold()
    _write_g11(tmp_path, g)
    for prefix, build in (('tag', build_user_and_item_tag_matrix), ('pop', build_user_and_item_pop_matrix)):
        user_mtx, item_mtx = build(str(tmp_path))
        assert user_mtx.dtype == torch.float32 and item_mtx.dtype == torch.float32
        assert np.array_equal(item_mtx.numpy(), g[f'item_{prefix}']), prefix
        assert np.array_equal(user_mtx.numpy(), g[f'user_{prefix}']), prefix      # the same numpy / scipy calls
        with pytest.raises(AssertionError, match='Alpha value out of bounds'):
            build(str(tmp_path), alpha_smoothening=1.5)
    item_tag = g['item_tag']
    assert not item_tag[:7].any() and np.allclose(item_tag[7:].sum(1), 1) and (np.count_nonzero(item_tag, 1) > 1).any()
    assert np.array_equal(g['item_pop'].sum(1), np.ones(200)) and (g['item_pop'].sum(0) > 0).all()
    assert np.isfinite(g['user_tag']).all() and (g['user_tag'].sum(1) <= 1 + 1e-6).all() and (g['user_tag'] > 0).all()
    assert np.allclose(g['user_pop'].sum(1), 1, atol=1e-6)
    # alpha = 0: the plain bucket frequencies of the user's train items
    user0, _ = build_user_and_item_pop_matrix(str(tmp_path), alpha_smoothening=0.)
    assert np.allclose(user0.numpy().sum(1), 1, atol=1e-6)


def test_builders_keep_nan_row_of_user_without_train_items(tmp_path):
    from hassaku_amd.data.data_utils import build_user_and_item_pop_matrix, build_user_and_item_tag_matrix
    g = _gold()
    _write_g11(tmp_path, g, drop_user=17)
    for prefix, build in (('tag', build_user_and_item_tag_matrix), ('pop', build_user_and_item_pop_matrix)):
        user_mtx, item_mtx = build(str(tmp_path))
        nan_rows = np.isnan(user_mtx.numpy()).all(1)
        assert nan_rows[17] and nan_rows.sum() == 1 and not np.isnan(user_mtx.numpy()[~nan_rows]).any(), prefix
        assert np.isfinite(item_mtx.numpy()).all()


def test_decorator_interface():
    import torch
    from hassaku_amd.algorithms import algorithms_utils as au
    from hassaku_amd.dist import evaluate_item_sharded
    from hassaku_amd.eval.eval import FullEvaluator, FullEvaluatorCalibrationDecorator
    g = _gold()
    groups = torch.from_numpy(g['user_group'])
    base = FullEvaluator(aggr_by_group=True, n_groups=2, user_to_user_group=groups)
    base.K_VALUES = [3, 7]
    ev = _nested(base, g)
    assert isinstance(ev, FullEvaluator) and ev.full_evaluator.full_evaluator is base
    assert ev.K_VALUES == [3, 7] and ev.full_evaluator.K_VALUES == [3, 7]          # of the innermost evaluator
    assert FullEvaluatorCalibrationDecorator.CALIBRATION_K_VALUES == [5, 10, 50, 100]
    assert ev.get_n_groups() == 2 and ev.get_user_to_user_group() is groups
    assert ev.metric_name_prefix == 'pop' and ev.full_evaluator.metric_name_prefix == 'tag' and ev.beta_smoothening == .01
    assert base.eval_topk(torch.arange(3), torch.zeros((3, 100), dtype=torch.int64)) is None and base.get_results() == {}
    user_mtx, item_mtx = _mats(g, 'tag')
    for beta in (-.1, 1.5):
        with pytest.raises(AssertionError, match='Beta value out of bounds'):
            FullEvaluatorCalibrationDecorator(base, item_mtx, user_mtx, beta_smoothening=beta)
    for beta in (0, 1):
        FullEvaluatorCalibrationDecorator(base, item_mtx, user_mtx, beta_smoothening=beta)
    with pytest.raises(ValueError, match='100 best items'):
        ev.eval_topk(torch.arange(3), torch.zeros((3, 50), dtype=torch.int64))
    with pytest.raises(ValueError, match='single-process evaluation'):
        evaluate_item_sharded(None, None, None, ev)
    # the model registry is what it was: calibration is a switch of the evaluation, not an algorithm
    assert 'p3alpha' in au.REGISTERED_ALGORITHM_NAMES and 'mf' in au.ALGORITHM_NAMES
    assert not any('calib' in n for n in au.REGISTERED_ALGORITHM_NAMES)


def test_symbol_declared_and_bound():
    from hassaku_amd import _lib
    header = open(os.path.join(REPO, 'include', 'hassaku_hip.h')).read()
    assert 'int hsk_calibration_metrics(const int32_t* topk_idx,' in header and '#define HSK_MAX_KS 8' in header
    restype, argtypes = _lib.SIGNATURES['hsk_calibration_metrics']
    decl = header[header.index('int hsk_calibration_metrics('):]
    decl = decl[:decl.index(');')]
    assert len(argtypes) == decl.count(',') + 1 == 18
    assert 'hsk_calib.hip' in open(os.path.join(REPO, 'hassaku_amd', 'csrc', 'Makefile')).read()
    if os.path.isfile(_lib.LIB_PATH):
        assert hasattr(_lib.load(), 'hsk_calibration_metrics')


def test_cli_lists_the_flag():
    out = subprocess.run([sys.executable, os.path.join(REPO, 'run_experiment.py'), '--help'], capture_output=True,
                         text=True, cwd=REPO, check=True).stdout
    assert '--measure_calibration' in out and '--conf_path' in out


# ------------------------------------------------------------------------------------------------------ GPU
N_ITEMS, N_USERS, R_MAX = 257, 37, 130
K_CONFIGS = [(100, (100, 50, 10, 5)), (100, (5, 10, 50, 100)), (5, (5,)), (7, (7, 1))]


@functools.lru_cache(maxsize=None)
def _kernel_inputs(n_bins):
    """Item rows of one to three bins with weights that sum to 1 (items 0-9 are zero rows; odd items never use the last
    bin, so a short list may leave it empty: kl = +inf, js = NaN at beta 0); user rows positive and normalised, users 1
    and 2 with exactly empty bins, user 5 NaN; lists with out-of-range ids: row 7 pads from rank 3 on, row 8 pads only, a -1 and
    an n_items in rows 9 and 10."""
    rng = np.random.RandomState(100 + n_bins)
    item = np.zeros((N_ITEMS, n_bins))
    for i in range(10, N_ITEMS):
        hi = n_bins - 1 if (i % 2 and n_bins > 1) else n_bins
        cols = rng.choice(hi, min(hi, rng.randint(1, 4)), replace=False)
        item[i, cols] = 1. / len(cols)
    user = rng.rand(N_USERS, n_bins) + .05
    user[1:3, 1:][rng.rand(2, n_bins - 1) < .3] = 0.            # users 1 and 2: some exactly empty bins (0 log 0 = NaN)
    user /= user.sum(1, keepdims=True)
    user[5] = np.nan
    ids = rng.randint(0, N_ITEMS, size=(R_MAX, 100)).astype(np.int32)
    ids[7, 3:] = PAD
    ids[8] = PAD
    ids[9, 2] = -1
    ids[10, 0] = N_ITEMS
    ids[11, :60] = np.arange(60) % 10            # zero rows only up to rank 60
    u = rng.randint(0, N_USERS, size=R_MAX).astype(np.int64)
    u[3], u[8], u[20], u[21] = 5, 0, 1, 2
    return item, user, ids, u


def _worst_ratio(dev, rs, what):
    """max |dev - restate| / (2^-52 S) over the finite entries, after the non-finite ones were held to kind and place"""
    _same_non_finite(dev, rs['value'], what)
    fin = np.isfinite(rs['value'])
    assert fin.any() or not np.isfinite(dev).any()
    with np.errstate(all='ignore'):
        diff = np.abs(cr.compared_of(dev) - rs['compared'])
        ratio = np.where(fin & (diff > 0), diff / (ULP * rs['scale']), 0.)
    assert not np.isnan(ratio).any(), what
    return float(ratio.max()) if ratio.size else 0.


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('n_bins', [1, 3, 18, 63, 64, 65, 300])
def test_kernel_vs_restatement(n_bins, dtype):
    import torch
    from hassaku_amd import hip_ops
    item, user, ids, u = _kernel_inputs(n_bins)
    item = item.astype(dtype)                                     # 1, 1/2, 1/3 rounded to the dtype: the input of both sides
    wide = torch.zeros((N_ITEMS, n_bins + 3), dtype=getattr(torch, dtype), device='cuda')
    wide[:, n_bins:] = 7.                                         # a leading dimension of n_bins + 3; the margin is never read
    wide[:, :n_bins] = torch.from_numpy(item).cuda()
    item_d, user_d = wide[:, :n_bins], torch.from_numpy(user).cuda()
    worst, n_inf, n_nan, n_fin = 0., 0, 0, 0
    for k_max, ks in K_CONFIGS:
        ids_k = np.ascontiguousarray(ids[:, :k_max])
        ids_d = torch.from_numpy(ids_k).cuda()
        for beta in (.01, 0., 1.):
            rs = cr.calibration(ids_k, u, item, user, beta, ks)
            for R in (1, 3, 4, 5, R_MAX):
                status = hip_ops.new_status('cuda')
                dev = hip_ops.calibration_metrics(ids_d[:R].contiguous(), torch.from_numpy(u[:R]).cuda(), item_d, user_d,
                                                  beta, ks, status=status)
                assert dev.shape == (R, len(ks), 3) and dev.dtype == torch.float64 and int(status.item()) == 0
                dev = dev.cpu().numpy()
                part = {name: a[:R] for name, a in rs.items()}
                worst = max(worst, _worst_ratio(dev, part, f'bins {n_bins} {dtype} k_max {k_max} ks {ks} beta {beta} R {R}'))
            n_inf += int(np.isposinf(dev).sum())
            n_nan += int(np.isnan(dev).sum())
            n_fin += int(np.isfinite(dev).sum())
            if beta == 1.:                                        # q = p: the distances are exactly 0 where p has no empty bin
                full = np.isfinite(rs['value']).all(axis=(1, 2))
                assert full.any() and not dev[full].any()
    print(f'bins {n_bins} {dtype}: worst |dev - restate| / (2^-52 S) = {worst:.2f}  (C = {C_KERNEL:g}); '
          f'at R = {R_MAX}: {n_fin} finite, {n_inf} +inf, {n_nan} NaN')
    assert n_nan > 0 and n_fin > 0 and n_inf > 0
    assert worst <= C_KERNEL
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize('tag', [t for t, _ in BETAS])
def test_kernel_vs_reference_golden(tag):
    import torch
    from hassaku_amd import hip_ops
    g = _gold()
    ids, users = torch.from_numpy(g['top_ids']).cuda(), torch.from_numpy(g['users']).cuda()
    got = {}
    for prefix in PREFIXES:
        user_mtx, item_mtx = _mats(g, prefix)
        met = hip_ops.calibration_metrics(ids, users, item_mtx.cuda(), user_mtx.double().cuda(), dict(BETAS)[tag], KS)
        met = met.cpu().numpy()
        got.update({f'{prefix}_{kind}@{k}': met[:, t, j] for t, k in enumerate(KS) for j, kind in enumerate(KINDS)})
    _hold_to_golden(got, g, tag, 'kernel')


@pytest.mark.gpu
def test_bad_arguments_and_bad_user_index():
    import torch
    from hassaku_amd import hip_ops
    item, user, ids, u = _kernel_inputs(18)
    item_d, user_d, ids_d = torch.from_numpy(item).cuda(), torch.from_numpy(user).cuda(), torch.from_numpy(ids).cuda()
    bad_u = u.copy()
    bad_u[[2, 77]] = [N_USERS, -1]
    status = hip_ops.new_status('cuda')
    dev = hip_ops.calibration_metrics(ids_d, torch.from_numpy(bad_u).cuda(), item_d, user_d, .01, KS, status=status)
    assert int(status.item()) == 1                               # HSK_STATUS_BAD_INDEX
    as_row0 = bad_u.copy()
    as_row0[[2, 77]] = 0
    ref = hip_ops.calibration_metrics(ids_d, torch.from_numpy(as_row0).cuda(), item_d, user_d, .01, KS)
    assert torch.equal(dev.nan_to_num(nan=-1.), ref.nan_to_num(nan=-1.))
    with pytest.raises(IndexError):
        hip_ops.raise_on_status(status, 'calibration')
    u_d = torch.from_numpy(u).cuda()
    for kw, err in ((dict(beta=1.5), RuntimeError), (dict(beta=float('nan')), RuntimeError), (dict(ks=[101]), RuntimeError),
                    (dict(ks=[0]), RuntimeError), (dict(ks=list(range(1, 10))), RuntimeError),
                    (dict(user=user_d.float()), TypeError), (dict(item=item_d.half()), TypeError),
                    (dict(ids=ids_d.long()), TypeError), (dict(user=user_d[:, :17].contiguous()), ValueError),
                    (dict(item=item_d.t().contiguous().t()), ValueError), (dict(u=u_d[:5]), ValueError)):
        with pytest.raises(err):
            hip_ops.calibration_metrics(kw.get('ids', ids_d), kw.get('u', u_d), kw.get('item', item_d),
                                        kw.get('user', user_d), kw.get('beta', .01), kw.get('ks', KS))
    wide = torch.from_numpy(np.ascontiguousarray(np.tile(ids, (1, 11))[:, :1025])).cuda()      # k_max above HSK_KNN_MAX_K
    with pytest.raises(RuntimeError, match='k_max'):
        hip_ops.calibration_metrics(wide, u_d, item_d, user_d, .01, KS)
    torch.cuda.synchronize()


def _evaluate_with_spy(model, loader, evaluator, device):
    """evaluate_recommender_algorithm, recording what the ranked paths hand to the outermost eval_topk"""
    from hassaku_amd.eval.eval import evaluate_recommender_algorithm
    seen = []
    inner = evaluator.eval_topk

    def spy(u_idxs, ids):
        seen.append((u_idxs.cpu().numpy().copy(), ids.cpu().numpy().copy()))
        inner(u_idxs, ids)
    evaluator.eval_topk = spy
    res = evaluate_recommender_algorithm(model, loader, evaluator, device)
    assert seen, 'the evaluation path never called eval_topk'
    return res, np.concatenate([s[0] for s in seen]), np.concatenate([s[1] for s in seen])


@pytest.mark.gpu
@pytest.mark.parametrize('alg', ['p3alpha', 'mf'])
def test_evaluation_with_nested_decorators(tmp_path, alg):
    """evaluate_recommender_algorithm with tag and pop decorators around the base evaluator on the g11 data, per user
    and aggregated with the two groups, against the restatement run on the ids the device itself selected."""
    import torch
    from hassaku_amd.data.data_utils import get_dataloader
    from hassaku_amd.data.dataset import TrainRecDataset
    from hassaku_amd.eval.eval import FullEvaluator
    g = _gold()
    _, path = _write_g11(tmp_path, g)
    loader = get_dataloader({'dataset_path': path, 'eval_batch_size': 64, 'running_settings': {'eval_n_workers': 0}}, 'val')
    if alg == 'p3alpha':
        from hassaku_amd.algorithms.graph_algs import P3alpha
        model = P3alpha(1.0)
        model.fit(TrainRecDataset(path).sampling_csr)
        device = model.device
    else:
        from hassaku_amd.algorithms.sgd_alg import SGDMatrixFactorization
        torch.manual_seed(3)
        model = SGDMatrixFactorization(300, 200, 32, False, True, False).to('cuda')
        device = 'cuda'
    plain = FullEvaluator(aggr_by_group=False)
    base_res, _, _ = _evaluate_with_spy(model, loader, plain, device)
    res, users, ids = _evaluate_with_spy(model, loader, _nested(FullEvaluator(aggr_by_group=False), g), device)
    assert np.array_equal(users, np.arange(300)) and ids.shape == (300, 100) and len(res) == 36
    assert all(np.array_equal(res[n], base_res[n]) for n in base_res)           # the base metrics are untouched
    worst = 0.
    per_user = {}
    for prefix in PREFIXES:
        rs = cr.calibration(ids, users, g[f'item_{prefix}'], g[f'user_{prefix}'], .01, KS)
        dev = np.stack([np.stack([res[f'{prefix}_{kind}@{k}'] for kind in KINDS], -1) for k in KS], 1)
        assert dev.dtype == np.float64 and np.isfinite(dev).all()
        worst = max(worst, _worst_ratio(dev, rs, f'{alg} {prefix}'))
        per_user[prefix] = dev
    print(f'{alg}: worst |dev - restate| / (2^-52 S) = {worst:.2f}  (C = {C_KERNEL:g})')
    assert worst <= C_KERNEL
    groups = g['user_group']
    ev = _nested(FullEvaluator(aggr_by_group=True, n_groups=2, user_to_user_group=torch.from_numpy(groups)), g)
    agg, _, ids2 = _evaluate_with_spy(model, loader, ev, device)
    assert np.array_equal(ids2, ids) and len(agg) == 3 * 36
    for prefix in PREFIXES:
        for gi, rows in ((None, np.ones(300, bool)), (0, groups == 0), (1, groups == 1)):
            for t, k in enumerate(KS):
                for j, kind in enumerate(KINDS):
                    name = ('' if gi is None else f'group_{gi}_') + f'{prefix}_{kind}@{k}'
                    want = per_user[prefix][rows, t, j].mean()               # the same kernel on the same ids: only the
                    assert abs(agg[name] - want) <= 300 * ULP * abs(want), name   # order of an fp64 sum of <= 300 differs
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize('logits_dtype', ['float32', 'float64'])
def test_dense_device_path_eval_batch(logits_dtype):
    """eval_batch of nested decorators on device logits (the path of the models scored densely): hsk_topk_dense for
    float32 logits, torch.topk otherwise, then the kernel; held to the golden, and equal to the ranked entry bit for bit."""
    import torch
    from hassaku_amd.eval.eval import FullEvaluator
    g = _gold()
    users = torch.from_numpy(g['users']).cuda()
    logits = _ranking_logits(g['top_ids'], g['labels'].shape[1]).to('cuda', getattr(torch, logits_dtype))
    labels = torch.from_numpy(g['labels'].astype(np.float32)).to('cuda', logits.dtype)
    for tag, beta in BETAS:
        ev = _nested(FullEvaluator(aggr_by_group=False), g, beta)
        ev.eval_batch(users, logits, labels)
        res = ev.get_results()
        assert len(res) == 36 and all(v.shape == (len(users),) for v in res.values())
        _hold_to_golden(res, g, tag, f'device eval_batch ({logits_dtype} logits)')
        ev.eval_topk(users, torch.from_numpy(g['top_ids']).cuda())
        ranked = ev.get_results()
        assert len(ranked) == 24 and all(np.array_equal(ranked[n], res[n], equal_nan=True) for n in ranked)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_decorated_device_path_allocates_no_gather():
    """One chunk through the ranked entry: nothing of the size of [rows, k, n_bins] (what the torch expressions gather) or
    [rows, n_items] may be allocated, and the matrices go to the device once."""
    import torch
    from hassaku_amd.eval.eval import FullEvaluator, FullEvaluatorCalibrationDecorator
    R, n_items, n_bins, n_users = 4096, 5000, 18, 4096
    rng = np.random.RandomState(0)
    item = torch.from_numpy((rng.rand(n_items, n_bins) < .1).astype(np.float32))
    user = torch.from_numpy(rng.dirichlet(np.ones(n_bins), n_users).astype(np.float32))
    ev = FullEvaluatorCalibrationDecorator(FullEvaluator(aggr_by_group=False), item, user)
    ids = torch.from_numpy(rng.randint(0, n_items, (R, 100)).astype(np.int32)).cuda()
    u = torch.arange(R, device='cuda')
    ev.eval_topk(u, ids)                                          # moves the matrices
    held = [t.data_ptr() for t in ev._on_device['cuda:0'][:2]]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    ev.eval_topk(u, ids)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    gather = R * 100 * n_bins * 4
    print(f'one chunk of {R} rows: {extra} bytes allocated at the peak; a [rows, k, n_bins] fp32 gather is {gather}, '
          f'[rows, n_items] fp32 {R * n_items * 4}')
    assert extra < gather // 8 and extra < R * n_items * 4 // 8
    assert [t.data_ptr() for t in ev._on_device['cuda:0'][:2]] == held and len(ev._on_device) == 1
    res = ev.get_results()
    assert len(res) == 12 and all(v.shape == (2 * R,) for v in res.values())       # both chunks, per user
    assert all(np.isfinite(v).all() for n, v in res.items() if 'hellinger' in n)


@pytest.mark.gpu
def test_run_test_with_measure_calibration(tmp_path):
    """run_experiment's path with the switch: the validation metrics are what they were, the test metrics carry the 24
    extra keys of each prefix, for everyone and for each group."""
    from hassaku_amd.algorithms.algorithms_utils import AlgorithmsEnum
    from hassaku_amd.data.data_utils import DatasetsEnum
    from hassaku_amd.experiment_helper import run_test, run_train_val
    g = _gold()
    _write_g11(tmp_path / 'data' / 'ml100k', g)
    conf = {'data_path': str(tmp_path / 'data'), 'model_save_path': str(tmp_path / 'models'), 'alpha': 1.0,
            'eval_batch_size': 64, 'running_settings': {'use_wandb': False, 'batch_verbose': False}}
    best, conf = run_train_val(AlgorithmsEnum['p3alpha'], DatasetsEnum.ml100k, conf)
    assert len(best) == 36
    plain = run_test(AlgorithmsEnum['p3alpha'], DatasetsEnum.ml100k, conf)
    conf['measure_calibration'] = True
    test = run_test(AlgorithmsEnum['p3alpha'], DatasetsEnum.ml100k, conf)
    assert len(plain) == 36 and len(test) == 3 * 36 and all(test[n] == plain[n] for n in plain)
    for prefix in PREFIXES:
        keys = [f'{prefix}_{kind}@{k}' for k in KS for kind in KINDS]
        assert len(keys) == 12
        for group in ('', 'group_0_', 'group_1_'):
            vals = np.array([test[group + n] for n in keys])
            assert np.isfinite(vals).all() and (vals > 0).all(), (prefix, group)
        everyone = np.array([test[n] for n in keys])
        n0, n1 = np.bincount(g['user_group'])
        mixed = (n0 * np.array([test['group_0_' + n] for n in keys]) + n1 * np.array([test['group_1_' + n] for n in keys])) / 300
        assert np.allclose(everyone, mixed, rtol=1e-12, atol=0)
