#!/usr/bin/env python3
"""Wall-clock timing of ECF on the HIP device at the synthetic ml1m and ml10m shapes: one training step (forward of
the model, BPR loss, backward; no optimiser step) and one full evaluation (item representations once, then every user
in batches against all items, scores only), and where the step's time goes:

  affiliation   `hip_ops.ecf_affiliation` forward + backward on the item block [n_items, C] and on the batch [B, C],
                next to the same operator composed from torch ops (topk, scatter, softmax, sigmoid, elementwise)
  gather-sums   `hip_ops.sparse_rows_sum` forward + backward: the batch's rows of X against x_tilde, and the tags' rows
                of the transposed incidence against the item affiliations (one wave sums a whole tag: `longest tag`)
  rest          the step minus the four pieces above: cosine GEMM, embedding lookups, losses

    python tools/ecf_timing.py [--shapes ml1m,ml10m] [--dim 100] [--clusters 64] [--top 20] [--tags 1000]
                               [--batch 256] [--neg 4] [--eval-batch 1024] [--step-timeout 600]

Tags are synthetic: three per item, drawn with a Zipf-like popularity, so a few tags hold thousands of items.  Each
shape runs in a fresh child process under its own `timeout` with at most 16 CPU threads; a shape that fails ends the
run.  After WARMUP calls, a sample is the mean of INNER back-to-back calls bracketed by torch.cuda.synchronize(); the
medians of REPEATS samples are reported.  The backward of a gather-sum includes its one host read-back.  Prints one JSON
line per shape.
"""
import argparse
import json
import os
import subprocess
import sys
import time

MAX_THREADS = 16
WARMUP, INNER, REPEATS = 3, 10, 9


def _threads() -> int:
    return min(MAX_THREADS, int(os.environ.get('OMP_NUM_THREADS') or MAX_THREADS))


def worker(opts):
    import numpy as np
    import torch
    from scipy import sparse as sp

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from hassaku_amd import hip_ops
    from hassaku_amd.algorithms.ecf_alg import ECF
    from hassaku_amd.data.csr import UserItemCsr
    from hassaku_amd.data.synthetic import generate_named
    from hassaku_amd.train.rec_losses import RecBayesianPersonalizedRankingLoss

    torch.set_num_threads(_threads())
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)

    def timed(fn):
        for _ in range(WARMUP):
            fn()
        samples = []
        for _ in range(REPEATS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(INNER):
                fn()
            torch.cuda.synchronize()
            samples.append((time.perf_counter() - t0) / INNER)
        return float(np.median(samples)) * 1e6

    d = generate_named(opts.shape, seed=0)
    U, I, C, k = d.n_users, d.n_items, opts.clusters, opts.top
    X = UserItemCsr.from_pairs(d.train[:, 0], d.train[:, 1], U, I)
    rng = np.random.RandomState(0)
    share = np.arange(1, opts.tags + 1, dtype=np.float64) ** -1.0
    tags = rng.choice(opts.tags, size=(I, 3), p=share / share.sum())
    inc = sp.csr_matrix((np.ones(3 * I), (np.repeat(np.arange(I), 3), tags.reshape(-1))), shape=(I, opts.tags))
    inc.sum_duplicates()
    inc.data[:] = 1.
    freq = np.asarray(inc.sum(0)).ravel()
    torch.manual_seed(0)
    model = ECF(U, I, inc @ sp.diags(np.log(I / (freq + 1e-6))), X, opts.dim, C, k, k).to(dev)
    loss_fn = RecBayesianPersonalizedRankingLoss()
    pick = rng.randint(0, len(d.train), opts.batch)
    u = torch.from_numpy(d.train[pick, 0].astype(np.int64)).to(dev)
    i = torch.from_numpy(np.concatenate([d.train[pick, 1:2], rng.randint(0, I, (opts.batch, opts.neg))], 1)
                         .astype(np.int64)).to(dev)
    labels = torch.zeros(i.shape, device=dev)
    labels[:, 0] = 1.

    def step():
        for p in model.parameters():
            p.grad = None
        out = model(u, i)
        (loss_fn.compute_loss(out, labels) + model.get_and_reset_other_loss()['reg_loss']).backward()

    def evaluation():
        with torch.no_grad():
            i_repr = model.get_item_representations(torch.arange(I, device=dev))
            for start in range(0, U, opts.eval_batch):
                users = torch.arange(start, min(start + opts.eval_batch, U), device=dev)
                model.combine_user_item_representations(model.get_user_representations(users), i_repr)

    def torch_affiliation(S, top, temp):
        m = torch.zeros_like(S)
        m[torch.arange(S.shape[0], device=S.device)[:, None], S.topk(top).indices] = 1.
        p = torch.softmax(S / temp, dim=-1)
        return torch.sigmoid(S) * (p + (m - p).detach())

    def fwd_bwd(fn, leaf, g):
        def run():
            leaf.grad = None
            fn(leaf).backward(g)
        return run

    out = {'shape': opts.shape, 'n_users': U, 'n_items': I, 'nnz_train': int(X.nnz), 'n_tags': opts.tags,
           'longest_tag': int(freq.max()), 'dim': opts.dim, 'clusters': C, 'top': k, 'batch': opts.batch,
           'neg': opts.neg, 'eval_batch': opts.eval_batch, 'warmup': WARMUP, 'inner': INNER, 'repeats': REPEATS}
    out['step_us'] = timed(step)
    out['eval_us'] = timed(evaluation)
    status = hip_ops.new_status(dev)
    x_tilde = (torch.rand(I, C, device=dev) * 2 - 1).requires_grad_()
    a_tilde = (torch.rand(opts.batch, C, device=dev) * 8).requires_grad_()
    g_items, g_batch = torch.randn(I, C, device=dev), torch.randn(opts.batch, C, device=dev)
    g_tags = torch.randn(opts.tags, C, device=dev)
    temp = model.temp_masking
    pieces = {
        'affiliation_items': fwd_bwd(lambda s: hip_ops.ecf_affiliation(s, k, temp), x_tilde, g_items),
        'affiliation_batch': fwd_bwd(lambda s: hip_ops.ecf_affiliation(s, k, temp), a_tilde, g_batch),
        'torch_affiliation_items': fwd_bwd(lambda s: torch_affiliation(s, k, temp), x_tilde, g_items),
        'torch_affiliation_batch': fwd_bwd(lambda s: torch_affiliation(s, k, temp), a_tilde, g_batch),
        'gather_users': fwd_bwd(lambda s: hip_ops.sparse_rows_sum(s, (model.x_indptr, model.x_indices), u, status),
                                x_tilde, g_batch),
        'gather_tags': fwd_bwd(lambda s: hip_ops.sparse_rows_sum(s, (model.tag_indptr, model.tag_indices),
                                                                 model.tag_rows, status), x_tilde, g_tags),
    }
    for name, fn in pieces.items():
        out[name + '_us'] = timed(fn)
    hip_ops.raise_on_status(status, 'ecf_timing')
    model.check_indices()
    own = ('affiliation_items', 'affiliation_batch', 'gather_users', 'gather_tags')
    out['rest_us'] = out['step_us'] - sum(out[n + '_us'] for n in own)
    for what in ('items', 'batch'):
        out[f'torch_over_hip_affiliation_{what}'] = out[f'torch_affiliation_{what}_us'] / out[f'affiliation_{what}_us']
    print(json.dumps({key: (round(v, 2) if isinstance(v, float) else v) for key, v in out.items()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='ml1m,ml10m')
    ap.add_argument('--dim', type=int, default=100)
    ap.add_argument('--clusters', type=int, default=64)
    ap.add_argument('--top', type=int, default=20)
    ap.add_argument('--tags', type=int, default=1000)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--neg', type=int, default=4)
    ap.add_argument('--eval-batch', type=int, default=1024)
    ap.add_argument('--step-timeout', type=int, default=600, help='seconds each shape may take')
    ap.add_argument('--shape', help=argparse.SUPPRESS)         # set by the driver: time this one shape in this process
    opts = ap.parse_args()
    if opts.shape:
        worker(opts)
        return 0
    env = dict(os.environ)
    for var in ('OMP_NUM_THREADS', 'MKL_NUM_THREADS', 'OPENBLAS_NUM_THREADS'):
        env[var] = str(_threads())
    for shape in opts.shapes.split(','):
        cmd = ['timeout', '-k', '10', str(opts.step_timeout), sys.executable, os.path.abspath(__file__), '--shape', shape]
        for flag in ('dim', 'clusters', 'top', 'tags', 'batch', 'neg', 'eval_batch'):
            cmd += ['--' + flag.replace('_', '-'), str(getattr(opts, flag))]
        rc = subprocess.run(cmd, env=env).returncode
        if rc != 0:
            print(f'{shape}: exit status {rc}; nothing more is started', file=sys.stderr)
            return rc
    return 0


if __name__ == '__main__':
    sys.exit(main())
