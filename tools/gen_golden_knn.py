"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/g11_knn_*.npz by running the reference's ItemKNN / UserKNN.

Runs only where the reference tree is available (imported unmodified with the stand-ins of SURVEY.md section 8c,
oracle/gen_golden.py:import_reference); the fixtures are committed, the reference never travels.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_knn.py

Dataset (g11_knn_data.npz): a synthetic 300 users x 200 items set (hassaku_amd.data.synthetic, 2 user groups):
its train / val / test pairs and the evaluated users (EVAL_USERS val users).
Per (alg, similarity) g11_knn_<alg>_<sim>.npz, for shrinkage s in {0, 10}, keys prefixed `s<s>.`:
  neigh_indptr / neigh_indices / neigh_data   compute_similarity_top_k's CSR at k = K_GOLD, rows in stored order
  pred                                        the reference's pred_mtx rows of the evaluated users (float64)
  top_vals / top_ids                          torch.topk(100) of those rows with the train items set to -inf
  gap                                         per user: 100th and 101st masked scores differ
  metric_names / metrics                      the reference FullEvaluator's per-user metrics of those users
"""
import os
import sys
import tempfile
from functools import partial

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle.gen_golden import OUT, import_reference, toy_dataset  # noqa: E402

K_GOLD = 20
EVAL_USERS = 48
SHRINKS = (0., 10.)
SIM_PARAMS = {'cosine': {}, 'jaccard': {}, 'sorensen_dice': {}, 'asymmetric_cosine': {'alpha': 0.3},
              'tversky': {'alpha': 0.7, 'beta': 0.4}}


def main():
    import_reference()
    from algorithms.knn_algs import ItemKNN, UserKNN
    from data.dataset import FullEvalDataset, TrainRecDataset
    from eval.eval import FullEvaluator
    from utilities.similarities import SimilarityFunctionEnum, compute_similarity_top_k

    with tempfile.TemporaryDirectory() as tmp:
        data = toy_dataset(tmp, n_users=300, n_items=200, n_inter=6000, n_groups=2, seed=11)
        train = TrainRecDataset(tmp)
        X = train.sampling_matrix
        val = FullEvalDataset(tmp, 'val')
        users = np.sort(np.random.RandomState(5).choice(data.n_users, EVAL_USERS, replace=False)).astype(np.int64)
        np.savez_compressed(os.path.join(OUT, 'g11_knn_data.npz'), n_users=data.n_users, n_items=data.n_items,
                            train=data.train, val=data.val, test=data.test, user_group=data.user_group,
                            users=users, k=K_GOLD, sim_params=np.array(repr(SIM_PARAMS)))
        excl = val.exclude_data.toarray()[users]
        labels = val.iteration_matrix.toarray()[users].astype(np.float32)
        for alg_name, cls in (('iknn', ItemKNN), ('uknn', UserKNN)):
            for sim, params in SIM_PARAMS.items():
                fx = {}
                for s in SHRINKS:
                    model = cls(SimilarityFunctionEnum[sim], K_GOLD, s, **params)
                    model.fit(X)
                    entity = X.T.tocsr() if alg_name == 'iknn' else X
                    S = compute_similarity_top_k(entity, model.sim_func, K_GOLD, s, model.BLOCK_SIZE)
                    pred = model.pred_mtx.toarray()[users].astype(np.float64)
                    masked = torch.from_numpy(pred.copy())
                    masked[torch.from_numpy(excl)] = -torch.inf
                    top = masked.topk(101)
                    ev = FullEvaluator(aggr_by_group=False, n_groups=0)
                    ev.eval_batch(torch.from_numpy(users), masked, torch.from_numpy(labels))
                    res = ev.get_results()
                    names = sorted(res)
                    p = f's{int(s)}.'
                    fx.update({p + 'neigh_indptr': S.indptr.astype(np.int64), p + 'neigh_indices': S.indices.astype(np.int32),
                               p + 'neigh_data': S.data.astype(np.float64), p + 'pred': pred,
                               p + 'top_vals': top.values[:, :100].numpy(), p + 'top_ids': top.indices[:, :100].numpy(),
                               p + 'gap': (top.values[:, 99] != top.values[:, 100]).numpy(),
                               p + 'metric_names': np.array(names),
                               p + 'metrics': np.stack([np.asarray(res[n], np.float64) for n in names], 1)})
                path = os.path.join(OUT, f'g11_knn_{alg_name}_{sim}.npz')
                np.savez_compressed(path, **fx)
                print(path, os.path.getsize(path))


if __name__ == '__main__':
    main()
