"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/g17_ecf.npz by running the reference's ECF
(algorithms/sgd_alg.py:579-775) on the CPU.

Runs only where the reference tree is available (imported unmodified with the stand-ins of SURVEY.md section 8c,
oracle/gen_golden.py:import_reference); the fixture is committed, the reference never travels.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_ecf.py

Dataset: the one of g11_knn_data.npz (300 users x 200 items, the same 48 evaluated users), regenerated from the same
seed and checked against that file, plus tag_idxs.csv / item_tag_idxs.csv written here: 12 tags, every tag used, no two
tags with the same item set, some items without a tag.  SciPy 1.15 has no `.A` on sparse matrices and the reference's
constructor reads it: the constructor is handed stand-ins whose `.A` is the dense array.

  n_users / n_items / n_tags / item_tag [n, 2] / tag_matrix [n_items, n_tags] float64 (the reference dataset's, dense)
  embedding_dim / temp_masking / temp_tags / top_p / lam = (lam_cf, lam_ind, lam_ts)
  eval.u [48]
and per block b in (c24: n_clusters 24, top_n = top_m = 5;  c64: n_clusters 64, top_n = top_m = 20):
  <b>.n_clusters / top_n / top_m / model_seed / batch_seed
  <b>.init.<key>         user_embed.weight, item_embed.weight, clusters after the seeded construction
  <b>.u_idx [B], <b>.i_idx [B, 1 + neg]      B = 16, neg = 4; user 1 repeats user 0, item (1, 0) item (0, 0)
  <b>.x_tilde, xs [n_items, C], a [B, C], scores [B, 1 + neg], cf_loss, ind_loss, ts_loss (weighted by lam)
  <b>.grad.<key>         gradients of bpr(scores) + reg_loss
  <b>.eval.scores [48, n_items]
  <b>.gap.x_tilde / a_tilde / eval_a_tilde / log_b      the smallest distance between the last value inside and the
                         first outside each discrete choice (top_m, top_n, top_n for the evaluated users, top_p)
  <b>.dist.<quantity>    max |reference - float64 restatement| / max |restatement| (tests/ecf_restate.py): the
                         reference's own fp32 error, against which the device tolerances are set

A model seed whose x_tilde / tag log-softmax / evaluated users' a_tilde has a gap below 1e-4, or a batch seed with a
user without a train item or an a_tilde gap below 1e-4, is skipped for the next one, and the script says so: rounding
must not flip a discrete choice, or the comparison would measure nothing.
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
from oracle.gen_golden import OUT, import_reference, toy_dataset  # noqa: E402

import ecf_restate  # noqa: E402

D, TOP_P, N_TAGS = 20, 3, 12
BLOCKS = (('c24', 24, 5), ('c64', 64, 20))
B, NEG = 16, 4
CLEAR = 1e-4


def write_tags(folder, n_items, seed=17):
    """12 tags with a skewed popularity, 0..3 per item; returns the [n, 2] (item, tag) pairs."""
    import pandas as pd
    rng = np.random.RandomState(seed)
    share = np.arange(1, N_TAGS + 1, dtype=np.float64) ** -0.7
    share /= share.sum()
    pairs = []
    for item in range(n_items):
        for tag in rng.choice(N_TAGS, size=rng.randint(0, 4), replace=False, p=share):
            pairs.append((item, int(tag)))
    pairs = np.asarray(sorted(pairs), np.int64)
    dense = np.zeros((n_items, N_TAGS), bool)
    dense[pairs[:, 0], pairs[:, 1]] = True
    assert dense.any(0).all(), 'a tag without items'
    assert len({dense[:, t].tobytes() for t in range(N_TAGS)}) == N_TAGS, 'two tags with the same item set'
    assert (~dense.any(1)).any(), 'every item has a tag'
    pd.DataFrame({'tag_idx': np.arange(N_TAGS), 'tag': [f't{t}' for t in range(N_TAGS)]}).to_csv(
        os.path.join(folder, 'tag_idxs.csv'), index=False)
    pd.DataFrame({'item_idx': pairs[:, 0], 'tag_idx': pairs[:, 1]}).to_csv(
        os.path.join(folder, 'item_tag_idxs.csv'), index=False)
    return pairs


def kth_gap(rows: np.ndarray, k: int) -> float:
    """min over rows of (k-th largest - (k+1)-th largest); inf when k is the row length."""
    if k >= rows.shape[-1]:
        return float('inf')
    s = -np.sort(-rows, axis=-1)
    return float((s[:, k - 1] - s[:, k]).min())


def draw_batch(seed, n_users, n_items):
    rng = np.random.RandomState(seed)
    u = rng.randint(0, n_users, size=B).astype(np.int64)
    i = rng.randint(0, n_items, size=(B, NEG + 1)).astype(np.int64)
    u[1] = u[0]
    i[1, 0] = i[0, 0]
    return torch.from_numpy(u), torch.from_numpy(i)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    den = np.abs(b).max()
    return float(np.abs(a - b).max() / (den if den > 0 else 1.0))


def main():
    import_reference()
    from algorithms.sgd_alg import ECF
    from data.dataset import ECFTrainRecDataset
    from train.rec_losses import RecBayesianPersonalizedRankingLoss

    g11 = np.load(os.path.join(OUT, 'g11_knn_data.npz'))
    limit = max(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT) if f.endswith('.npz'))
    with tempfile.TemporaryDirectory() as tmp:
        data = toy_dataset(tmp, n_users=300, n_items=200, n_inter=6000, n_groups=2, seed=11)
        assert np.array_equal(data.train, g11['train']) and np.array_equal(data.val, g11['val'])
        pairs = write_tags(tmp, 200)
        train = ECFTrainRecDataset(tmp)
    X = np.asarray(train.sampling_matrix.todense()).astype(np.float64)
    T = np.asarray(train.tag_matrix.todense()).astype(np.float64)
    assert set(np.unique(X)) <= {0, 1}
    n_users, n_items = X.shape
    users = np.sort(np.random.RandomState(5).choice(n_users, 48, replace=False)).astype(np.int64)
    assert np.array_equal(users, g11['users'])
    lam = None
    fx = {'n_users': np.int64(n_users), 'n_items': np.int64(n_items), 'n_tags': np.int64(N_TAGS), 'item_tag': pairs,
          'tag_matrix': T, 'embedding_dim': np.int64(D), 'top_p': np.int64(TOP_P), 'eval.u': users}
    X64, T64 = torch.from_numpy(X), torch.from_numpy(T)
    loss_fn = RecBayesianPersonalizedRankingLoss()
    for name, C, k in BLOCKS:
        model_seed = 64
        while True:
            torch.manual_seed(model_seed)
            model = ECF(n_users, n_items, types.SimpleNamespace(A=T), types.SimpleNamespace(A=X), embedding_dim=D,
                        n_clusters=C, top_n=k, top_m=k, top_p=TOP_P)
            assert sorted(model.state_dict()) == ['clusters', 'item_embed.weight', 'user_embed.weight']
            with torch.no_grad():
                model._generate_item_representations()
                x_tilde = model._x_tildes.numpy()
                log_b = torch.log_softmax(model._xs.T @ model.tag_matrix / model.temp_tags, -1).numpy()
                gaps = {'x_tilde': kth_gap(x_tilde, k), 'log_b': kth_gap(log_b, TOP_P),
                        'eval_a_tilde': kth_gap(X[users].astype(np.float32) @ x_tilde, k)}
            if min(gaps.values()) >= CLEAR:
                break
            print(f'{name}: model seed {model_seed} leaves gaps {gaps}, trying seed {model_seed + 1}')
            model_seed += 1
        init = {key: v.detach().numpy().copy() for key, v in model.state_dict().items()}
        batch_seed = 3
        while True:
            u, i = draw_batch(batch_seed, n_users, n_items)
            a_tilde = X[u.numpy()].astype(np.float32) @ x_tilde
            gaps['a_tilde'] = kth_gap(a_tilde, k)
            if X[u.numpy()].sum(1).min() > 0 and gaps['a_tilde'] >= CLEAR:
                break
            print(f'{name}: batch seed {batch_seed} has a user without train items or an a_tilde gap '
                  f"{gaps['a_tilde']:.3g}, trying seed {batch_seed + 1}")
            batch_seed += 1
        labels = torch.zeros((B, NEG + 1))
        labels[:, 0] = 1.
        scores = model(u, i)
        other = model.get_and_reset_other_loss()
        (loss_fn.compute_loss(scores, labels) + other['reg_loss']).backward()
        got = {'x_tilde': model._x_tildes, 'xs': model._xs, 'a': model.get_user_representations(u)[0],
               'scores': scores, 'cf_loss': other['cf_loss'], 'ind_loss': other['ind_loss'],
               'ts_loss': other['ts_loss']}
        got = {key: v.detach().numpy().copy() for key, v in got.items()}
        for pname, p in model.named_parameters():
            if p.requires_grad:
                assert p.grad is not None and float(p.grad.abs().max()) > 0, pname
                got['grad.' + pname] = p.grad.numpy().copy()
        with torch.no_grad():     # evaluation form: item representations once, then the users against all of them
            i_repr = model.get_item_representations(torch.arange(n_items))
            got['eval.scores'] = (model.get_user_representations(torch.from_numpy(users))[0] @ i_repr[0].T).numpy().copy()
        lam = np.asarray([model.lam_cf, model.lam_ind, model.lam_ts])

        # the float64 restatement on the same state and batch
        leaves = {key: torch.from_numpy(v).double().requires_grad_() for key, v in init.items()}
        args = (leaves['user_embed.weight'], leaves['item_embed.weight'], leaves['clusters'], X64, T64)
        hyper = (k, k, model.temp_masking, model.temp_tags, TOP_P)
        r = ecf_restate.forward_f64(*args, u, i, *hyper)
        reg = lam[2] * r['ts'] + lam[1] * r['ind'] + lam[0] * r['cf']
        (ecf_restate.bpr(r['scores']) + reg).backward()
        want = {'x_tilde': r['x_tilde'], 'xs': r['xs'], 'a': r['a'], 'scores': r['scores'], 'cf_loss': lam[0] * r['cf'],
                'ind_loss': lam[1] * r['ind'], 'ts_loss': lam[2] * r['ts']}
        want = {key: v.detach().numpy() for key, v in want.items()}
        for key, leaf in leaves.items():
            want['grad.' + key] = leaf.grad.numpy()
        with torch.no_grad():
            want['eval.scores'] = ecf_restate.forward_f64(*args, torch.from_numpy(users), torch.arange(n_items),
                                                          *hyper)['scores'].numpy()
        assert np.array_equal(got['xs'] != 0, want['xs'] != 0) and np.array_equal(got['a'] != 0, want['a'] != 0)
        fx.update({f'{name}.n_clusters': np.int64(C), f'{name}.top_n': np.int64(k), f'{name}.top_m': np.int64(k),
                   f'{name}.model_seed': np.int64(model_seed), f'{name}.batch_seed': np.int64(batch_seed),
                   f'{name}.u_idx': u.numpy(), f'{name}.i_idx': i.numpy()})
        for key, v in init.items():
            fx[f'{name}.init.{key}'] = v
        for key, v in gaps.items():
            fx[f'{name}.gap.{key}'] = np.float64(v)
        for key, v in got.items():
            fx[f'{name}.{key}'] = v
            fx[f'{name}.dist.{key}'] = np.float64(rel(v, want[key]))
            print(f'{name}: {key:24s} reference vs float64 restatement {fx[f"{name}.dist.{key}"]:.3e}')
        print(f'{name}: model seed {model_seed}, batch seed {batch_seed}, gaps', {g: f'{v:.3g}' for g, v in gaps.items()})
    fx.update({'temp_masking': np.float64(model.temp_masking), 'temp_tags': np.float64(model.temp_tags), 'lam': lam})
    path = os.path.join(OUT, 'g17_ecf.npz')
    np.savez_compressed(path, **fx)
    size = os.path.getsize(path)
    print(path, size)
    assert size <= limit, (path, size, limit)


if __name__ == '__main__':
    main()
