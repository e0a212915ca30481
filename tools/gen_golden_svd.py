"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/g14_svd_k*.npz by running the reference's SVDAlgorithm
(scipy.sparse.linalg.svds).

Runs only where the reference tree is available (imported unmodified with the stand-ins of SURVEY.md section 8c,
oracle/gen_golden.py:import_reference); the fixtures are committed, the reference never travels.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_svd.py

Dataset: the one of g11_knn_data.npz (tools/gen_golden_knn.py: 300 users x 200 items, 2 user groups, the same 48
evaluated users), regenerated from the same seed and checked against that file.
Per n_factors in FACTORS, g14_svd_k<n_factors>.npz:
  n_factors               the value handed to the reference
  singular_values         the column norms of the reference's users_factors (= U S), descending
  pred                    users_factors @ items_factors.T, the rows of the evaluated users (float64, dense)
  top_vals / top_ids      torch.topk(100) of those rows with the train items set to -inf
  metric_names / metrics  the reference FullEvaluator's per-user metrics of those users
  users_factors / items_factors   (k8 only) the reference's own factors, in its column order and signs
The reference's fit() casts with `asfptype()`, which turns its int16 sampling matrix into float32, so on its own data
path svds runs in single precision (singular values off by ~4e-6).  The model here is float64, and the bounds of
tests/test_svd.py are derived for a float64 reference, so the matrix is handed over as float64 (`asfptype()` then keeps
it): the same class, the same svds call, in double precision.
It also confirms what svds demands of k: 1 <= k < min(shape).
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
FACTORS = (8, 16, 100)


def main():
    import_reference()
    from algorithms.mf_algs import SVDAlgorithm
    from data.dataset import FullEvalDataset, TrainRecDataset
    from eval.eval import FullEvaluator

    g11 = np.load(os.path.join(OUT, 'g11_knn_data.npz'))
    limit = max(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT) if f.startswith('g11_knn_'))
    with tempfile.TemporaryDirectory() as tmp:
        data = toy_dataset(tmp, n_users=300, n_items=200, n_inter=6000, n_groups=2, seed=11)
        assert np.array_equal(data.train, g11['train']) and np.array_equal(data.val, g11['val'])
        train = TrainRecDataset(tmp)
        X = train.sampling_matrix.astype(np.float64)
        val = FullEvalDataset(tmp, 'val')
        users = np.sort(np.random.RandomState(5).choice(data.n_users, EVAL_USERS, replace=False)).astype(np.int64)
        assert np.array_equal(users, g11['users'])
        excl = val.exclude_data.toarray()[users]
        labels = val.iteration_matrix.toarray()[users].astype(np.float32)
        for bad in (0, min(X.shape)):
            try:
                SVDAlgorithm(bad).fit(X)
            except ValueError as e:
                print(f'svds refuses k = {bad}: {e}')
            else:
                raise AssertionError(f'svds accepted k = {bad}')
        for k in FACTORS:
            model = SVDAlgorithm(k)
            model.fit(X)
            uf, vf = model.users_factors, np.ascontiguousarray(model.items_factors)
            assert uf.dtype == np.float64 and vf.dtype == np.float64
            assert uf.shape == (data.n_users, k) and vf.shape == (data.n_items, k)
            pred = uf[users] @ vf.T
            assert np.isfinite(pred).all()
            masked = torch.from_numpy(pred.copy())
            masked[torch.from_numpy(excl)] = -torch.inf
            top = masked.topk(100)
            ev = FullEvaluator(aggr_by_group=False, n_groups=0)
            ev.eval_batch(torch.from_numpy(users), masked, torch.from_numpy(labels))
            res = ev.get_results()
            names = sorted(res)
            fx = {'n_factors': np.int64(k), 'singular_values': np.sort(np.sqrt((uf * uf).sum(0)))[::-1].copy(),
                  'pred': pred, 'top_vals': top.values.numpy(), 'top_ids': top.indices.numpy(),
                  'metric_names': np.array(names),
                  'metrics': np.stack([np.asarray(res[n], np.float64) for n in names], 1)}
            if k == FACTORS[0]:
                fx.update(users_factors=uf, items_factors=vf)
            path = os.path.join(OUT, f'g14_svd_k{k}.npz')
            np.savez_compressed(path, **fx)
            size = os.path.getsize(path)
            print(path, size)
            assert size <= limit, (path, size, limit)


if __name__ == '__main__':
    main()
