#!/usr/bin/env python3
"""Wall-clock timing of the sparse first layer of DeepMatrixFactorization on the HIP device at the synthetic ml1m shape
(6040 x 3706, 1 M interactions, of which the train split is used), batch 64 x (1 + 4), hidden width 64 and 128: one
forward + backward of each tower's first layer through `hip_ops.sparse_rows_sum`, next to the reference's formulation on
the same device -- the dense fp32 train matrix (and its transpose) as a frozen nn.Embedding feeding nn.Linear.

    python tools/dmf_timing.py [--shapes ml1m] [--widths 64,128] [--batch 64] [--neg 4] [--step-timeout 600]

The user tower sees `batch` row ids, the item tower batch x (1 + neg) column ids (positives drawn from the train pairs,
negatives uniform), as in a training step.  Each shape runs in a fresh child process under its own `timeout`; a shape
that fails ends the run.  After WARMUP calls, a sample is the mean of INNER back-to-back forward + backward calls
bracketed by torch.cuda.synchronize(); the two paths alternate sample by sample, and the medians of REPEATS samples are
reported with their minimum and maximum.  The backward of the sparse path includes its one host read-back (the batch's
entry count).  Memory: the bytes each path keeps resident for its input (the CSR of X and of X^T against the two dense
fp32 copies); the first-layer weights are the same size in both.  Prints one JSON line per shape.
"""
import argparse
import json
import os
import subprocess
import sys
import time

MAX_THREADS = 16
WARMUP, INNER, REPEATS = 5, 50, 15


def _threads() -> int:
    return min(MAX_THREADS, int(os.environ.get('OMP_NUM_THREADS') or MAX_THREADS))


def worker(opts):
    import numpy as np
    import torch
    from torch import nn

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from hassaku_amd import hip_ops
    from hassaku_amd.algorithms.base_classes import csr_transpose
    from hassaku_amd.data.csr import UserItemCsr
    from hassaku_amd.data.synthetic import generate_named

    torch.set_num_threads(_threads())
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)

    def now():
        torch.cuda.synchronize()
        return time.perf_counter()

    d = generate_named(opts.shape, seed=0)
    train = UserItemCsr.from_pairs(d.train[:, 0], d.train[:, 1], d.n_users, d.n_items)
    n_users, n_items, nnz = d.n_users, d.n_items, int(train.nnz)
    x_ptr, x_idx = train.to_device(dev)
    t_ptr, t_idx, _ = csr_transpose(x_ptr, x_idx, None, n_users, n_items)
    dense = torch.zeros((n_users, n_items), dtype=torch.float32, device=dev)
    dense[torch.repeat_interleave(torch.arange(n_users, device=dev), x_ptr[1:] - x_ptr[:-1]), x_idx.long()] = 1
    user_vectors = nn.Embedding.from_pretrained(dense)
    item_vectors = nn.Embedding.from_pretrained(dense.T.contiguous())
    rng = np.random.RandomState(0)
    pick = rng.randint(0, len(d.train), opts.batch)
    u_idx = torch.from_numpy(d.train[pick, 0].astype(np.int64)).to(dev)
    i_idx = torch.from_numpy(np.concatenate([d.train[pick, 1:2], rng.randint(0, n_items, (opts.batch, opts.neg))],
                                            1).astype(np.int64)).to(dev)
    out = {'shape': opts.shape, 'n_users': n_users, 'n_items': n_items, 'nnz_train': nnz, 'batch': opts.batch,
           'neg': opts.neg, 'warmup': WARMUP, 'inner': INNER, 'repeats': REPEATS,
           'sparse_input_bytes': sum(t.numel() * t.element_size() for t in (x_ptr, x_idx, t_ptr, t_idx)),
           'dense_input_bytes': 2 * dense.numel() * 4}
    for width in (int(w) for w in opts.widths.split(',')):
        for side, csr, vectors, idx, n_in in (('user', (x_ptr, x_idx), user_vectors, u_idx, n_items),
                                              ('item', (t_ptr, t_idx), item_vectors, i_idx, n_users)):
            torch.manual_seed(0)
            lin = nn.Linear(n_in, width).to(dev)
            Wt = lin.weight.detach().t().contiguous().requires_grad_()
            bias = lin.bias.detach().clone().requires_grad_()
            g = torch.randn(tuple(idx.shape) + (width,), device=dev)
            status = hip_ops.new_status(dev)

            def sparse():
                Wt.grad = bias.grad = None
                (hip_ops.sparse_rows_sum(Wt, csr, idx, status) + bias).backward(g)

            def dense_path():
                lin.weight.grad = lin.bias.grad = None
                lin(vectors(idx)).backward(g)

            sparse()
            dense_path()
            diff = float((Wt.grad.T - lin.weight.grad).abs().max() / lin.weight.grad.abs().max())
            for _ in range(WARMUP):
                sparse()
                dense_path()
            samples = {'sparse': [], 'dense': []}
            for _ in range(REPEATS):
                for name, fn in (('sparse', sparse), ('dense', dense_path)):
                    t0 = now()
                    for _ in range(INNER):
                        fn()
                    samples[name].append((now() - t0) / INNER)
            hip_ops.raise_on_status(status, 'dmf_timing')
            key = f'{side}_h{width}'
            out[key + '_rows'] = int(idx.numel())
            out[key + '_entries'] = int((csr[0][idx.reshape(-1) + 1] - csr[0][idx.reshape(-1)]).sum())
            out[key + '_grad_max_rel_diff'] = diff
            for name, xs in samples.items():
                out[f'{key}_{name}_us'] = float(np.median(xs)) * 1e6
                out[f'{key}_{name}_min_us'] = min(xs) * 1e6
                out[f'{key}_{name}_max_us'] = max(xs) * 1e6
    print(json.dumps({k: (round(v, 3) if isinstance(v, float) and abs(v) > 1e-3 else v) for k, v in out.items()}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='ml1m')
    ap.add_argument('--widths', default='64,128')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--neg', type=int, default=4)
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
        cmd = ['timeout', '-k', '10', str(opts.step_timeout), sys.executable, os.path.abspath(__file__), '--shape', shape,
               '--widths', opts.widths, '--batch', str(opts.batch), '--neg', str(opts.neg)]
        rc = subprocess.run(cmd, env=env).returncode
        if rc != 0:
            print(f'{shape}: exit status {rc}; nothing more is started', file=sys.stderr)
            return rc
    return 0


if __name__ == '__main__':
    sys.exit(main())
