"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/g16_calibration.npz by running the reference's calibration layer:
build_user_and_item_tag_matrix / build_user_and_item_pop_matrix (data/data_utils.py:378-498) and
FullEvaluatorCalibrationDecorator (eval/eval.py:121-208).

Runs only where the reference tree is available (imported unmodified with the stand-ins of SURVEY.md section 8c,
oracle/gen_golden.py:import_reference, plus the `.A` of sparse matrices that scipy 1.14 dropped); the fixture is
committed, the reference never travels.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_calibration.py

Dataset: the one of g11_knn_data.npz (300 users x 200 items, 6000 interactions, 2 user groups, seed 11) written under
<tmp>/processed_dataset, plus tag_idxs.csv (18 tags) and a seeded item_tag_idxs.csv: items 0-6 carry no tag, every
other item one to three.  No model is run: the ranked lists are the top_ids of g13_p3alpha_a1p0.npz (the same 48
evaluated users), handed to the decorator as logits that rank exactly those ids in that order.

g16_calibration.npz:
  user_tag / item_tag / user_pop / item_pop   the reference's four matrices (float32)
  item_tags, n_tags                           the (item_idx, tag_idx) pairs of item_tag_idxs.csv and the tag count
  users, top_ids, labels, user_group          the evaluated users, their ranked ids [48, 100], their validation label
                                              rows (uint8) and every user's group
  ks, names                                   the cut-offs and the per-user metric names (tag_* then pop_*)
  per_user_b0p01 / per_user_b0                the reference's per-user metrics (aggr_by_group=False) at beta .01 / 0,
                                              float32 [48, len(names)], columns in the order of `names`
  aggr_names / aggr_values                    the aggregated dictionary with the two groups at beta .01
  fp32_err_b0p01 / fp32_err_b0                what the reference's float32 arithmetic costs on this very fixture: worst
                                              |reference - fp64 restatement (tests/calibration_restate.py)| over the
                                              finite entries, [prefix (tag, pop), 4]: hellinger, jensen-shannon (rows
                                              with fp64 js^2 >= 1e-6), kl, and js^2 (rows below 1e-6).  The tests
                                              take four times these as their bound against the golden.
"""
import os
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
from oracle.gen_golden import OUT, import_reference, toy_dataset  # noqa: E402

N_TAGS = 18
UNTAGGED = 7            # items 0 .. 6
KS = [5, 10, 50, 100]
BETAS = (('b0p01', .01), ('b0', 0.))
JS2_SMALL = 1e-6
PREFIXES = ('tag', 'pop')
KINDS = ('hellinger_distance', 'jensen_shannon_distance', 'kl_divergence')


def item_tag_pairs(n_items):
    rng = np.random.RandomState(16)
    pairs = []
    for item in range(UNTAGGED, n_items):
        n = rng.choice([1, 1, 1, 2, 2, 3])
        pairs += [(item, int(t)) for t in np.sort(rng.choice(N_TAGS, n, replace=False))]
    return np.asarray(pairs, np.int64)


def ranking_logits(top_ids, n_items):
    """float32 logits whose top-100 are exactly top_ids, in order"""
    logits = torch.full((top_ids.shape[0], n_items), -1., dtype=torch.float32)
    k = top_ids.shape[1]
    logits.scatter_(1, torch.from_numpy(top_ids.astype(np.int64)),
                    torch.arange(k, 0, -1, dtype=torch.float32).expand(top_ids.shape[0], k).contiguous())
    assert np.array_equal(logits.topk(k).indices.numpy(), top_ids)
    return logits


def fp32_cost(ref, users, top_ids, mats, beta):
    """[prefix, 4] worst |reference float32 - restatement float64| (see the module docstring)"""
    import calibration_restate as cr
    out = np.zeros((len(PREFIXES), 4))
    for pi, prefix in enumerate(PREFIXES):
        user_mtx, item_mtx = mats[prefix]
        rs = cr.calibration(top_ids, users, item_mtx.numpy(), user_mtx.numpy(), beta, KS)
        for t, k in enumerate(KS):
            for j, kind in enumerate(KINDS):
                got = np.asarray(ref[f'{prefix}_{kind}@{k}'], np.float64)
                want = rs['value'][:, t, j]
                assert np.array_equal(np.isnan(got), np.isnan(want)), (prefix, kind, k)
                assert np.array_equal(np.isposinf(got), np.isposinf(want)) and not np.isneginf(got).any()
                fin = np.isfinite(want)
                if kind == 'jensen_shannon_distance':
                    small = fin & (rs['compared'][:, t, j] < JS2_SMALL)
                    fin &= ~small
                    if small.any():
                        out[pi, 3] = max(out[pi, 3], np.abs(got[small] ** 2 - rs['compared'][small, t, j]).max())
                if fin.any():
                    out[pi, j] = max(out[pi, j], np.abs(got[fin] - want[fin]).max())
    return out


def main():
    import_reference()
    from scipy import sparse as sp
    for cls in (sp.csr_matrix, sp.csc_matrix, sp.coo_matrix):
        if not hasattr(cls, 'A'):
            cls.A = property(lambda self: self.toarray())
    from data.data_utils import build_user_and_item_pop_matrix, build_user_and_item_tag_matrix
    from data.dataset import FullEvalDataset
    from eval.eval import FullEvaluator, FullEvaluatorCalibrationDecorator
    import pandas as pd

    g11 = np.load(os.path.join(OUT, 'g11_knn_data.npz'))
    g13 = np.load(os.path.join(OUT, 'g13_p3alpha_a1p0.npz'))
    users, top_ids = g11['users'].astype(np.int64), g13['top_ids'].astype(np.int64)
    with tempfile.TemporaryDirectory() as tmp:
        folder = os.path.join(tmp, 'processed_dataset')
        data = toy_dataset(folder, n_users=300, n_items=200, n_inter=6000, n_groups=2, seed=11)
        assert np.array_equal(data.train, g11['train']) and np.array_equal(data.val, g11['val'])
        pairs = item_tag_pairs(data.n_items)
        pd.DataFrame({'tag_idx': np.arange(N_TAGS)}).to_csv(os.path.join(folder, 'tag_idxs.csv'), index=False)
        pd.DataFrame({'item_idx': pairs[:, 0], 'tag_idx': pairs[:, 1]}).to_csv(
            os.path.join(folder, 'item_tag_idxs.csv'), index=False)
        mats = {'tag': build_user_and_item_tag_matrix(tmp), 'pop': build_user_and_item_pop_matrix(tmp)}
        val = FullEvalDataset(folder, 'val')
        labels = torch.from_numpy(val.iteration_matrix.toarray()[users].astype(np.float32))
        groups = val.user_to_user_group
        n_groups = val.n_user_groups
    for user_mtx, item_mtx in mats.values():
        assert user_mtx.dtype == torch.float32 and item_mtx.dtype == torch.float32
    assert not mats['tag'][1][:UNTAGGED].any() and (mats['tag'][1][UNTAGGED:].sum(1) > 0).all()
    logits = ranking_logits(top_ids, data.n_items)
    u = torch.from_numpy(users)

    def run(aggr, beta):
        ev = FullEvaluator(aggr_by_group=aggr, n_groups=n_groups if aggr else 0,
                           user_to_user_group=groups if aggr else None)
        for prefix in PREFIXES:
            ev = FullEvaluatorCalibrationDecorator(ev, mats[prefix][1], mats[prefix][0], metric_name_prefix=prefix,
                                                   beta_smoothening=beta)
        ev.eval_batch(u, logits.clone(), labels)
        return ev.get_results()

    names = [f'{p}_{kind}@{k}' for p in PREFIXES for k in KS for kind in KINDS]
    fx = {'user_tag': mats['tag'][0].numpy(), 'item_tag': mats['tag'][1].numpy(), 'user_pop': mats['pop'][0].numpy(),
          'item_pop': mats['pop'][1].numpy(), 'item_tags': pairs, 'n_tags': np.int64(N_TAGS), 'users': users,
          'top_ids': top_ids.astype(np.int32), 'labels': labels.numpy().astype(np.uint8),
          'user_group': groups.numpy().astype(np.int64), 'ks': np.asarray(KS), 'names': np.array(names)}
    for tag, beta in BETAS:
        res = run(False, beta)
        assert set(names) <= set(res)
        assert all(np.asarray(res[n]).dtype == np.float32 for n in names)
        fx[f'per_user_{tag}'] = np.stack([np.asarray(res[n]) for n in names], 1)
        fx[f'fp32_err_{tag}'] = fp32_cost(res, users, top_ids, mats, beta)
        print(tag, 'non-finite', int((~np.isfinite(fx[f'per_user_{tag}'])).sum()), 'of', fx[f'per_user_{tag}'].size)
        print(tag, 'fp32 cost [prefix, (hel, js, kl, js2 small)]\n', fx[f'fp32_err_{tag}'])
    res = run(True, .01)
    aggr_names = sorted(res)
    fx['aggr_names'] = np.array(aggr_names)
    fx['aggr_values'] = np.asarray([res[n] for n in aggr_names], np.float64)
    path = os.path.join(OUT, 'g16_calibration.npz')
    np.savez_compressed(path, **fx)
    print(path, os.path.getsize(path), 'bytes;', len(aggr_names), 'aggregated keys')
    assert os.path.getsize(path) <= 400 * 1024


if __name__ == '__main__':
    main()
