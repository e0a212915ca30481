"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/g12_ease_*.npz by running the reference's EASE.

Runs only where the reference tree is available (imported unmodified with the stand-ins of SURVEY.md section 8c,
oracle/gen_golden.py:import_reference); the fixtures are committed, the reference never travels.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_ease.py

Dataset: the one of g11_knn_data.npz (tools/gen_golden_knn.py: 300 users x 200 items, 2 user groups, the same 48
evaluated users), regenerated from the same seed and checked against that file.
Per lam in LAMS, g12_ease_lam<lam>.npz (50.7 is written as lam50p7: the reference truncates it to 50):
  lam                     the value handed to the reference
  pred                    the reference's pred_mtx rows of the evaluated users (float64)
  top_vals / top_ids      torch.topk(100) of those rows with the train items set to -inf
  gap                     per user: 100th and 101st masked scores differ
  metric_names / metrics  the reference FullEvaluator's per-user metrics of those users
For lam = 50 the reference's B in full, recomputed with its own five lines on the same matrix and checked to give its
pred_mtx bitwise; it is split by rows over g12_ease_lam50_B0.npz / _B1.npz so that no file outgrows the largest g11
fixture.
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
LAMS = (1, 50, 500, 50.7)


def lam_tag(lam):
    return str(lam).replace('.', 'p')


def main():
    import_reference()
    from algorithms.linear_algs import EASE
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
        for lam in LAMS:
            model = EASE(lam)
            model.fit(X)
            pred = np.asarray(model.pred_mtx)[users].astype(np.float64)
            masked = torch.from_numpy(pred.copy())
            masked[torch.from_numpy(excl)] = -torch.inf
            top = masked.topk(101)
            ev = FullEvaluator(aggr_by_group=False, n_groups=0)
            ev.eval_batch(torch.from_numpy(users), masked, torch.from_numpy(labels))
            res = ev.get_results()
            names = sorted(res)
            fx = {'lam': np.float64(lam), 'pred': pred, 'top_vals': top.values[:, :100].numpy(),
                  'top_ids': top.indices[:, :100].numpy(), 'gap': (top.values[:, 99] != top.values[:, 100]).numpy(),
                  'metric_names': np.array(names),
                  'metrics': np.stack([np.asarray(res[n], np.float64) for n in names], 1)}
            files = {f'g12_ease_lam{lam_tag(lam)}.npz': fx}
            if lam == 50:
                G = X.transpose().dot(X).toarray()
                G[np.diag_indices(G.shape[0])] += int(lam)
                P = np.linalg.inv(G)
                B = P / (-np.diag(P))
                B[np.diag_indices(G.shape[0])] = 0
                assert np.array_equal(np.asarray(X @ B), np.asarray(model.pred_mtx))
                half = B.shape[0] // 2
                files['g12_ease_lam50_B0.npz'] = {'row0': np.int64(0), 'B': B[:half]}
                files['g12_ease_lam50_B1.npz'] = {'row0': np.int64(half), 'B': B[half:]}
            for name, arrays in files.items():
                path = os.path.join(OUT, name)
                np.savez_compressed(path, **arrays)
                size = os.path.getsize(path)
                print(path, size)
                assert size <= limit, (name, size, limit)


if __name__ == '__main__':
    main()
