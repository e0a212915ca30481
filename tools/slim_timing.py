#!/usr/bin/env python3
"""Wall-clock timing of SLIM on the HIP device at the synthetic ml1m and ml10m shapes: one whole fit, the solver
(hsk_slim_cd_f64) alone on the same Gram, and what the solver worked on: the candidates per column (g_i > l1, d_i > 0,
i != j), how many columns had more of them than fit in LDS, the sweeps run and the weights kept.

    python tools/slim_timing.py [--shapes ml1m,ml10m] [--alpha 0.01] [--l1-ratio 0.3] [--max-iter 50]

Each phase is bracketed by torch.cuda.synchronize(); one warm-up fit precedes the timed one.  Prints one JSON line per
shape.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hassaku_amd import hip_ops  # noqa: E402
from hassaku_amd.algorithms.base_classes import csr_arrays  # noqa: E402
from hassaku_amd.algorithms.linear_algs import SLIM  # noqa: E402
from hassaku_amd.data.csr import UserItemCsr  # noqa: E402
from hassaku_amd.data.synthetic import generate_named  # noqa: E402


def _now():
    torch.cuda.synchronize()
    return time.perf_counter()


def candidate_counts(G, l1, rows=1024):
    n = G.shape[0]
    held = torch.diagonal(G) > 0
    counts = torch.empty(n, dtype=torch.int64, device=G.device)
    for r0 in range(0, n, rows):
        blk = (G[r0:r0 + rows] > l1) & held[None, :]
        idx = torch.arange(r0, min(r0 + rows, n), device=G.device)
        blk[idx - r0, idx] = False
        counts[r0:r0 + rows] = blk.sum(1)
    return counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='ml1m,ml10m')
    ap.add_argument('--alpha', type=float, default=0.01)
    ap.add_argument('--l1-ratio', type=float, default=0.3)
    ap.add_argument('--max-iter', type=int, default=50)
    opts = ap.parse_args()
    torch.cuda.set_device(0)
    for shape in opts.shapes.split(','):
        d = generate_named(shape, seed=0)
        train = UserItemCsr.from_pairs(d.train[:, 0], d.train[:, 1], d.n_users, d.n_items)
        model = SLIM(opts.alpha, opts.l1_ratio, opts.max_iter)
        model.fit(train)                       # warm-up
        t0 = _now()
        model.fit(train)
        fit_total = _now() - t0
        n_iter, W = model.n_iter_, model.W
        out = {'shape': shape, 'alpha': opts.alpha, 'l1_ratio': opts.l1_ratio, 'max_iter': opts.max_iter,
               'tol': model.tol, 'n_users': d.n_users, 'n_items': d.n_items, 'nnz_train': int(train.nnz),
               'fit_s': fit_total, 'sweeps_mean': float(n_iter.double().mean()), 'sweeps_max': int(n_iter.max()),
               'columns_at_max_iter': int((n_iter == opts.max_iter).sum()),
               'weights_kept': int((W > 0).sum()), 'weights_per_column_mean': float((W > 0).sum(0).double().mean())}
        model.W = W = None
        torch.cuda.empty_cache()
        G, _ = model._gram(*csr_arrays(train), 0)      # the phase methods SLIM.fit calls
        l1, l2 = model.penalties(d.n_users)
        t0 = _now()
        model._solve(G, d.n_users)
        out['solver_s'] = _now() - t0
        counts = candidate_counts(G, l1)
        out.update(l1=l1, l2=l2, candidates_mean=float(counts.double().mean()), candidates_max=int(counts.max()),
                   lds_candidates=hip_ops.SLIM_LDS_CANDIDATES,
                   columns_beyond_lds=int((counts > hip_ops.SLIM_LDS_CANDIDATES).sum()))
        print(json.dumps({k: (round(v, 6) if isinstance(v, float) else v) for k, v in out.items()}), flush=True)
        del model, G
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
