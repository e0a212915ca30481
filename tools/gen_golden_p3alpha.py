"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/g13_p3alpha_*.npz by running the reference's P3alpha.

Runs only where the reference tree is available (imported unmodified with the stand-ins of SURVEY.md section 8c,
oracle/gen_golden.py:import_reference); the fixtures are committed, the reference never travels.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_p3alpha.py

Dataset: the one of g11_knn_data.npz (tools/gen_golden_knn.py: 300 users x 200 items, 2 user groups, the same 48
evaluated users), regenerated from the same seed and checked against that file.
Per alpha in ALPHAS, g13_p3alpha_a<alpha>.npz (1.9 is written as a1p9):
  alpha                   the value handed to the reference
  pred                    the reference's pred_mtx rows of the evaluated users (float64, dense)
  top_vals / top_ids      torch.topk(100) of those rows with the train items set to -inf
  gap                     per user: 100th and 101st masked scores differ
  metric_names / metrics  the reference FullEvaluator's per-user metrics of those users
"""
import os
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle.gen_golden import OUT, import_reference, toy_dataset  # noqa: E402

EVAL_USERS = 48
ALPHAS = (1.9, 1.0, 0.5)


def alpha_tag(alpha):
    return str(alpha).replace('.', 'p')


def main():
    import_reference()
    from algorithms.graph_algs import P3alpha
    from data.dataset import FullEvalDataset, TrainRecDataset
    from eval.eval import FullEvaluator

    g11 = np.load(os.path.join(OUT, 'g11_knn_data.npz'))
    limit = max(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT) if f.startswith('g11_knn_'))
    with tempfile.TemporaryDirectory() as tmp:
        data = toy_dataset(tmp, n_users=300, n_items=200, n_inter=6000, n_groups=2, seed=11)
        assert np.array_equal(data.train, g11['train']) and np.array_equal(data.val, g11['val'])
        train = TrainRecDataset(tmp)
        X = train.sampling_matrix
        val = FullEvalDataset(tmp, 'val')
        users = np.sort(np.random.RandomState(5).choice(data.n_users, EVAL_USERS, replace=False)).astype(np.int64)
        assert np.array_equal(users, g11['users'])
        excl = val.exclude_data.toarray()[users]
        labels = val.iteration_matrix.toarray()[users].astype(np.float32)
        for alpha in ALPHAS:
            model = P3alpha(alpha)
            model.fit(X)
            pred = np.asarray(model.pred_mtx[users].todense()).astype(np.float64)
            assert np.isfinite(pred).all()
            masked = torch.from_numpy(pred.copy())
            masked[torch.from_numpy(excl)] = -torch.inf
            top = masked.topk(101)
            ev = FullEvaluator(aggr_by_group=False, n_groups=0)
            ev.eval_batch(torch.from_numpy(users), masked, torch.from_numpy(labels))
            res = ev.get_results()
            names = sorted(res)
            fx = {'alpha': np.float64(alpha), 'pred': pred, 'top_vals': top.values[:, :100].numpy(),
                  'top_ids': top.indices[:, :100].numpy(), 'gap': (top.values[:, 99] != top.values[:, 100]).numpy(),
                  'metric_names': np.array(names),
                  'metrics': np.stack([np.asarray(res[n], np.float64) for n in names], 1)}
            path = os.path.join(OUT, f'g13_p3alpha_a{alpha_tag(alpha)}.npz')
            np.savez_compressed(path, **fx)
            size = os.path.getsize(path)
            print(path, size)
            assert size <= limit, (path, size, limit)


if __name__ == '__main__':
    main()
