#!/usr/bin/env python3
"""Wall-clock timing of EASE on the HIP device at the synthetic ml1m and ml10m shapes: fit by phase (pack / Gram /
inverse / weights), the full-catalogue scoring plus top-100, and numpy.linalg.inv of the same G on the host's CPUs.

    python tools/ease_timing.py [--shapes ml1m,ml10m] [--lam 100] [--no-cpu]

Each phase is bracketed by torch.cuda.synchronize(); one warm-up fit precedes the timed one.  The inverse's rate is
2 n^3 flop (the blocked Gauss-Jordan's multiply-adds, symmetry not exploited) over its time.  `fit_beats_numpy_inv`
is the condition the model is held to: the whole GPU fit takes less time than the CPU library's inverse alone.
Prints one JSON line per shape.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hassaku_amd import hip_ops  # noqa: E402
from hassaku_amd.algorithms.base_classes import csr_arrays  # noqa: E402
from hassaku_amd.algorithms.linear_algs import EASE  # noqa: E402
from hassaku_amd.data.csr import UserItemCsr  # noqa: E402
from hassaku_amd.data.synthetic import generate_named  # noqa: E402


def _now():
    torch.cuda.synchronize()
    return time.perf_counter()


def time_fit(model, train):
    """(phase -> seconds, G on the host before the inverse): the phase methods EASE.fit calls, timed one by one."""
    t0 = _now()
    _, _, M = model._pack(*csr_arrays(train))
    t1 = _now()
    G = model._gram_f64(M, train.n_cols, model.lam_int)
    t2 = _now()
    del M
    G_host = G.cpu().numpy()
    t3 = _now()
    model._inverse(G)
    t4 = _now()
    model._weights(G)
    t5 = _now()
    return {'pack_s': t1 - t0, 'gram_s': t2 - t1, 'inverse_s': t4 - t3, 'weights_s': t5 - t4}, G_host


def time_eval(model, train, chunk_bytes=1 << 29):
    dev = model.device
    ep, ei = train.to_device(dev)
    n_users, n_items = train.n_rows, train.n_cols
    chunk = max(1, min(n_users, chunk_bytes // (8 * n_items)))
    buf = torch.empty((chunk, n_items), dtype=torch.float64, device=dev)
    score = topk = 0.
    for lo in range(0, n_users, chunk):
        u = torch.arange(lo, min(lo + chunk, n_users), device=dev)
        a = _now()
        s = model.score_rows(u, excl=(ep, ei), out=buf[:len(u)])
        b = _now()
        hip_ops.knn_topk_rows(s, 100)
        c = _now()
        score += b - a
        topk += c - b
    model.check_indices()
    return {'score_s': score, 'topk_s': topk, 'eval_chunk': chunk}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='ml1m,ml10m')
    ap.add_argument('--lam', type=float, default=100)
    ap.add_argument('--no-cpu', action='store_true', help='skip numpy.linalg.inv on the host')
    opts = ap.parse_args()
    torch.cuda.set_device(0)
    for shape in opts.shapes.split(','):
        d = generate_named(shape, seed=0)
        train = UserItemCsr.from_pairs(d.train[:, 0], d.train[:, 1], d.n_users, d.n_items)
        n = d.n_items
        model = EASE(opts.lam)
        model.fit(train)                       # warm-up (and the model the eval timing uses)
        t0 = _now()
        model.fit(train)
        fit_total = _now() - t0
        ev = time_eval(model, train)
        model.B = None
        torch.cuda.empty_cache()
        phases, G = time_fit(model, train)
        out = {'shape': shape, 'lam': opts.lam, 'n_users': d.n_users, 'n_items': n, 'nnz_train': int(train.nnz),
               'fit_s': fit_total, **phases, **ev, 'inverse_flop': 2 * n ** 3,
               'inverse_fp64_flops': 2 * n ** 3 / phases['inverse_s']}
        if not opts.no_cpu:
            t0 = time.perf_counter()
            P = np.linalg.inv(G)
            out['numpy_inv_s'] = time.perf_counter() - t0
            out['numpy_inv_threads'] = int(os.environ.get('OMP_NUM_THREADS', os.cpu_count()))
            out['fit_beats_numpy_inv'] = bool(fit_total < out['numpy_inv_s'])
            del P
        print(json.dumps({k: (round(v, 6) if isinstance(v, float) else v) for k, v in out.items()}), flush=True)
        del model, G
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
