#!/usr/bin/env python3
"""Wall-clock timing of P3alpha on the HIP device at the synthetic ml1m and ml10m shapes: one whole fit, its steps one
by one (pack / degrees / Gram), the full-catalogue scoring plus top-100, and scipy's sparse X^T diag(w_u) X -> dense on
the host's CPUs.

    python tools/p3alpha_timing.py [--shapes ml1m,ml10m] [--alpha 1.9] [--no-cpu] [--step-timeout 900]

Each shape runs in a fresh child process under its own `timeout`; a shape that fails ends the run.  At most 16 host
threads are used.  Each phase is bracketed by torch.cuda.synchronize(); one warm-up fit precedes the timed ones, and
`fit_s` is the median of five fits (`fit_min_s` / `fit_max_s` give the spread).  The Gram's rate is
2 n_items^2 k_pad flop (the padded k of the int8 operand, symmetry not exploited) over its time, printed next to the
chip's fp64 matrix peak (78.6 Tflop/s, AMD's MI355X data sheet) and the 18.5 Tflop/s measured inside k_ease_update
(MEASUREMENTS.md, "EASE timings").  `fit_beats_scipy_gram` is the condition the model is held to: the whole GPU fit
takes less time than the host's sparse product alone.  (The reference's own form, (P @ P) @ P on the
(users + items)^2 transition matrix, cannot serve as the comparator: at ml10m it builds a users x users product of
about 58 GB.)  Prints one JSON line per shape.
"""
import argparse
import json
import os
import subprocess
import sys
import time

MAX_THREADS = 16
FIT_REPEATS = 5
FP64_MATRIX_PEAK = 78.6e12
EASE_UPDATE_FLOPS = 18.5e12


def _threads() -> int:
    return min(MAX_THREADS, int(os.environ.get('OMP_NUM_THREADS') or MAX_THREADS))


def worker(opts):
    import numpy as np
    import scipy.sparse as sp
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from hassaku_amd import hip_ops
    from hassaku_amd.algorithms.graph_algs import P3alpha
    from hassaku_amd.algorithms.base_classes import csr_arrays
    from hassaku_amd.data.csr import UserItemCsr
    from hassaku_amd.data.synthetic import generate_named

    torch.set_num_threads(_threads())
    torch.cuda.set_device(0)

    def now():
        torch.cuda.synchronize()
        return time.perf_counter()

    d = generate_named(opts.shape, seed=0)
    train = UserItemCsr.from_pairs(d.train[:, 0], d.train[:, 1], d.n_users, d.n_items)
    n_users, n = d.n_users, d.n_items
    model = P3alpha(opts.alpha)
    model.fit(train)                       # warm-up (and the model the eval timing uses)
    fits = []
    for _ in range(FIT_REPEATS):
        t0 = now()
        model.fit(train)
        fits.append(now() - t0)
    fit_total = float(np.median(fits))

    # full-catalogue scoring with the train items at -inf, then top-100
    dev = model.device
    ep, ei = train.to_device(dev)
    chunk = max(1, min(n_users, (1 << 29) // (8 * n)))
    buf = torch.empty((chunk, n), dtype=torch.float64, device=dev)
    score = topk = 0.
    for lo in range(0, n_users, chunk):
        u = torch.arange(lo, min(lo + chunk, n_users), device=dev)
        a = now()
        s = model.score_rows(u, excl=(ep, ei), out=buf[:len(u)])
        b = now()
        hip_ops.knn_topk_rows(s, 100)
        c = now()
        score += b - a
        topk += c - b
    model.check_indices()
    model.W = None
    del buf
    torch.cuda.empty_cache()

    # the phase methods P3alpha.fit calls, one by one
    t0 = now()
    (x_ptr, _), t_ptr, M = model._pack(*csr_arrays(train))
    t1 = now()
    w_u, w_i = model._degrees(x_ptr, t_ptr, M.shape[1])
    t2 = now()
    W = model._weighted_gram(M, n, w_u, w_i)
    t3 = now()
    k_pad = int(M.shape[1])
    gram_flop = 2 * n * n * k_pad
    out = {'shape': opts.shape, 'alpha': opts.alpha, 'n_users': n_users, 'n_items': n, 'nnz_train': int(train.nnz),
           'k_pad': k_pad, 'fit_s': fit_total, 'fit_min_s': min(fits), 'fit_max_s': max(fits), 'pack_s': t1 - t0,
           'degrees_s': t2 - t1, 'gram_s': t3 - t2,
           'score_s': score, 'topk_s': topk, 'eval_chunk': chunk, 'gram_flop': gram_flop,
           'gram_fp64_flops': gram_flop / (t3 - t2), 'fp64_matrix_peak_flops': FP64_MATRIX_PEAK,
           'gram_of_peak': gram_flop / (t3 - t2) / FP64_MATRIX_PEAK, 'ease_update_fp64_flops': EASE_UPDATE_FLOPS}
    del M, W
    torch.cuda.empty_cache()
    if not opts.no_cpu:
        X = sp.csr_matrix((np.ones(train.nnz), train.indices, train.indptr), shape=(n_users, n))
        deg = np.diff(train.indptr)
        w = np.zeros(n_users)
        w[deg > 0] = 1.0 / deg[deg > 0]
        print(f'{opts.shape}: device steps done, timing the host product', file=sys.stderr, flush=True)
        t0 = time.perf_counter()
        S = (X.T @ sp.diags(w) @ X).toarray()
        out['scipy_gram_s'] = time.perf_counter() - t0
        out['host_threads'] = _threads()
        out['fit_beats_scipy_gram'] = bool(fit_total < out['scipy_gram_s'])
        del S
    print(json.dumps({k: (round(v, 6) if isinstance(v, float) else v) for k, v in out.items()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='ml1m,ml10m')
    ap.add_argument('--alpha', type=float, default=1.9)
    ap.add_argument('--no-cpu', action='store_true', help="skip scipy's sparse product on the host")
    ap.add_argument('--step-timeout', type=int, default=900, help='seconds each shape may take')
    ap.add_argument('--shape', help=argparse.SUPPRESS)         # set by the driver: time this one shape in this process
    opts = ap.parse_args()
    if opts.shape:
        worker(opts)
        return 0
    env = dict(os.environ)
    for var in ('OMP_NUM_THREADS', 'MKL_NUM_THREADS', 'OPENBLAS_NUM_THREADS'):
        env[var] = str(_threads())
    for shape in opts.shapes.split(','):
        cmd = ['timeout', '-k', '10', str(opts.step_timeout), sys.executable, os.path.abspath(__file__),
               '--shape', shape, '--alpha', str(opts.alpha)] + (['--no-cpu'] if opts.no_cpu else [])
        rc = subprocess.run(cmd, env=env).returncode
        if rc != 0:
            print(f'{shape}: exit status {rc}; nothing more is started', file=sys.stderr)
            return rc
    return 0


if __name__ == '__main__':
    sys.exit(main())
