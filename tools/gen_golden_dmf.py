"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/g15_dmf.npz by running the reference's DeepMatrixFactorization
(algorithms/sgd_alg.py:778-880) on the CPU.

Runs only where the reference tree is available (imported unmodified with the stand-ins of SURVEY.md section 8c,
oracle/gen_golden.py:import_reference); the fixture is committed, the reference never travels.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_dmf.py

Dataset: the one of g11_knn_data.npz (tools/gen_golden_knn.py: 300 users x 200 items, the same 48 evaluated users),
regenerated from the same seed and checked against that file.  The model is built after torch.manual_seed(64) with
u_mid_layers = [24, 20], i_mid_layers = 40, final_dimension = 12 on the train split's iteration matrix.

  n_users / n_items / lr / wd / u_mid_layers / i_mid_layers / final_dimension / batch_seed
  init.<key>         the tower parameters after the seeded construction, in the reference's shapes (the two dense
                     `*_vectors.weight` entries of its state dict are the train matrix and are not stored)
  s<k>.u_idx [B], s<k>.i_idx [B, 1 + neg]     B = 16, neg = 4, k = 1, 2; user 1 repeats user 0, item (1, 0) item (0, 0)
  s<k>.logits, s<k>.rec_loss                  forward and the reference's bce loss (the conf default)
  s1.grad.<key>      gradients of every tower parameter at step 1
  s<k>.param.<key>   tower parameters after each torch.optim.AdamW step
  eval.u, eval.scores    the 48 users x all items, evaluation form, after step 2

More than half of the scores sit on the floor mu = 1e-6 (the reference assigns mu where the cosine is smaller, and passes
no gradient there).  So no top-k or metric of the reference is stored: tie order would decide them.  And a difference at
rounding level must not move an entry of a training batch across the floor and switch its gradient: the generator
requires every cosine of the two batches to stay 1e-4 away from mu (on either side, which includes the golden logits
on the unclamped side); a batch that does not is redrawn from the next seed, and the script says so.
"""
import os
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle.gen_golden import OUT, import_reference, toy_dataset  # noqa: E402

U_MID, I_MID, FINAL = [24, 20], 40, 12
B, NEG, LR, WD = 16, 4, 1e-3, 1e-4
CLEAR = 1e-4   # distance every batch cosine keeps from mu


def tower_state(model):
    return {k: v.detach().numpy().copy() for k, v in model.state_dict().items()
            if k.startswith(('user_nn.', 'item_nn.'))}


def draw_batch(seed, n_users, n_items):
    rng = np.random.RandomState(seed)
    u = rng.randint(0, n_users, size=B).astype(np.int64)
    i = rng.randint(0, n_items, size=(B, NEG + 1)).astype(np.int64)
    u[1] = u[0]
    i[1, 0] = i[0, 0]
    return torch.from_numpy(u), torch.from_numpy(i)


def main():
    import_reference()
    from algorithms.sgd_alg import DeepMatrixFactorization
    from data.dataset import TrainRecDataset
    from train.rec_losses import RecBinaryCrossEntropy

    g11 = np.load(os.path.join(OUT, 'g11_knn_data.npz'))
    limit = max(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
    with tempfile.TemporaryDirectory() as tmp:
        data = toy_dataset(tmp, n_users=300, n_items=200, n_inter=6000, n_groups=2, seed=11)
        assert np.array_equal(data.train, g11['train']) and np.array_equal(data.val, g11['val'])
        train = TrainRecDataset(tmp)
        matrix = train.iteration_matrix
        dense = np.asarray(matrix.todense())
        assert set(np.unique(dense)) <= {0, 1}, 'the reference would feed values other than 0/1'
        print('longest user row', int(dense.sum(1).max()), 'longest item column', int(dense.sum(0).max()))
        torch.manual_seed(64)
        model = DeepMatrixFactorization(matrix, U_MID, I_MID, FINAL)
    n_users, n_items = dense.shape
    fx = {'n_users': np.int64(n_users), 'n_items': np.int64(n_items), 'lr': LR, 'wd': WD,
          'u_mid_layers': np.asarray(U_MID, np.int64), 'i_mid_layers': np.asarray([I_MID], np.int64),
          'final_dimension': np.int64(FINAL)}
    for k, v in tower_state(model).items():
        fx['init.' + k] = v
    loss_fn = RecBinaryCrossEntropy()
    opt = torch.optim.AdamW(model.parameters(), lr=LR, weight_decay=WD)
    seed = 3
    seeds = []
    for step in (1, 2):
        while True:
            u, i = draw_batch(seed, n_users, n_items)
            seed += 1
            with torch.no_grad():
                raw = model.cosine_func(model.get_user_representations(u)[:, None, :],
                                        model.get_item_representations(i))
            gap = float((raw - model.mu).abs().min())
            if gap > CLEAR:
                break
            print(f'step {step}: seed {seed - 1} puts a cosine {gap:.3g} from mu, redrawing from seed {seed}')
        seeds.append(seed - 1)
        labels = torch.zeros((B, NEG + 1), dtype=torch.float64)
        labels[:, 0] = 1.
        out = model(u, i)
        logits = out.detach().numpy().copy()
        free = logits[logits > model.mu]
        assert free.size and float((free - model.mu).min()) > CLEAR
        rec = loss_fn.compute_loss(out, labels)
        fx[f's{step}.u_idx'], fx[f's{step}.i_idx'] = u.numpy(), i.numpy()
        fx[f's{step}.logits'] = logits
        fx[f's{step}.rec_loss'] = np.float64(rec.item())
        rec.backward()
        if step == 1:
            for pname, p in model.named_parameters():
                if pname.startswith(('user_nn.', 'item_nn.')):
                    assert p.grad is not None and float(p.grad.abs().max()) > 0, pname
                    fx['s1.grad.' + pname] = p.grad.numpy().copy()
        opt.step()
        opt.zero_grad()
        for k, v in tower_state(model).items():
            fx[f's{step}.param.' + k] = v
        print(f'step {step}: seed {seeds[-1]}, rec_loss {rec.item():.6f}, '
              f'{float((logits <= model.mu).mean()):.2f} of the logits on the floor, nearest cosine {gap:.3g} from mu')
    fx['batch_seed'] = np.asarray(seeds, np.int64)
    users = np.sort(np.random.RandomState(5).choice(n_users, 48, replace=False)).astype(np.int64)
    assert np.array_equal(users, g11['users'])
    with torch.no_grad():   # evaluation form, eval/eval.py:237-248
        scores = model.combine_user_item_representations(model.get_user_representations(torch.from_numpy(users)),
                                                         model.get_item_representations(torch.arange(n_items)))
    fx['eval.u'] = users
    fx['eval.scores'] = scores.numpy().copy()
    print('eval:', float((fx['eval.scores'] <= model.mu).mean()), 'of the scores on the floor')
    path = os.path.join(OUT, 'g15_dmf.npz')
    np.savez_compressed(path, **fx)
    size = os.path.getsize(path)
    print(path, size)
    assert size <= limit, (path, size, limit)


if __name__ == '__main__':
    main()
