#!/usr/bin/env python3
"""Wall-clock timing of ItemKNN / UserKNN on the HIP device: fit (pack / Gram / select) and the full-catalogue
evaluation (score rows / top-100 / metrics) at the synthetic ml1m and ml10m shapes.

    python tools/knn_timing.py [--shapes ml1m,ml10m] [--algs iknn,uknn] [--k 100] [--sim cosine]

Each phase is bracketed by torch.cuda.synchronize(); one warm-up fit precedes the timed one.  The Gram's rate is
reported as int8 ops/s (2 * rows * n * k_pad per block, the padded operand's work) and as a fraction of 2x the bf16
dense peak (MI355X: 2.5 PFLOP/s bf16 dense -> 5.0 POPS int8).  Prints one JSON line per (shape, alg).
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
from hassaku_amd.algorithms.knn_algs import ItemKNN, UserKNN  # noqa: E402
from hassaku_amd.data.csr import UserItemCsr  # noqa: E402
from hassaku_amd.data.synthetic import generate_named  # noqa: E402

BF16_DENSE_PEAK = 2.5e15
I8_PEAK = 2 * BF16_DENSE_PEAK


def _now():
    torch.cuda.synchronize()
    return time.perf_counter()


def time_fit(model, train):
    """(phase -> seconds, gram int8 ops) of one fit: the phase methods KNNAlgorithm.fit calls, timed one by one."""
    t0 = _now()
    M, n_ent, degrees = model._pack(*csr_arrays(train))
    t1 = _now()
    gram = select = 0.
    ops = 0
    blocks = model._count_blocks(M, n_ent)
    while True:
        a = _now()
        block = next(blocks, None)        # one launch of the Gram kernel
        b = _now()
        if block is None:
            break
        r0, r1, C = block
        model._select(C, r0, r1, degrees)
        c = _now()
        gram += b - a
        select += c - b
        ops += 2 * (-(-(r1 - r0) // 128) * 128) * (-(-n_ent // 128) * 128) * M.shape[1]
    return {'pack_s': t1 - t0, 'gram_s': gram, 'select_s': select}, ops


def time_eval(model, train, excl_csr, chunk_bytes=1 << 29):
    dev = model.device
    ep, ei = excl_csr.to_device(dev)
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
    return {'score_s': score, 'topk_s': topk, 'eval_chunk': chunk}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='ml1m,ml10m')
    ap.add_argument('--algs', default='iknn,uknn')
    ap.add_argument('--k', type=int, default=100)
    ap.add_argument('--sim', default='cosine')
    opts = ap.parse_args()
    torch.cuda.set_device(0)
    for shape in opts.shapes.split(','):
        d = generate_named(shape, seed=0)
        train = UserItemCsr.from_pairs(d.train[:, 0], d.train[:, 1], d.n_users, d.n_items)
        for alg in opts.algs.split(','):
            model = (ItemKNN if alg == 'iknn' else UserKNN)(opts.sim, opts.k, 0.)
            model.fit(train)                       # warm-up (and the model the eval timing uses)
            t0 = _now()
            model.fit(train)
            fit_total = _now() - t0
            phases, ops = time_fit(model, train)
            ev = time_eval(model, train, train)
            out = {'shape': shape, 'alg': alg, 'sim': opts.sim, 'k': opts.k, 'n_users': d.n_users, 'n_items': d.n_items,
                   'nnz_train': int(train.nnz), 'fit_s': fit_total, **phases, **ev,
                   'gram_int8_ops': ops, 'gram_ops_per_s': ops / phases['gram_s'],
                   'gram_frac_of_2x_bf16_peak': ops / phases['gram_s'] / I8_PEAK}
            print(json.dumps({k: (round(v, 6) if isinstance(v, float) else v) for k, v in out.items()}), flush=True)
            del model
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
