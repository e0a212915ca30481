#!/usr/bin/env python3
"""Wall-clock timing of the ALS model on the HIP device: one fit on generate(3000, 1500, 150000, seed=3) (`s1500`) and
on the synthetic ml1m shape of bench.py (6040 x 3706; the train split of its interactions is fitted), at
k = 64 and k = 128 factors, and each half-sweep of an iteration on its own (the Gram and the solve, users and items).

    python tools/als_timing.py [--shapes s1500,ml1m] [--factors 64,128] [--n-iterations 4] [--step-timeout 600]

Each (shape, k) runs in a fresh child process under its own `timeout`; one that fails ends the run.  Each phase is
bracketed by torch.cuda.synchronize(); one warm-up fit precedes the timed ones and `fit_s` is the median of five fits.
A kernel's time is the mean of KERNEL_REPEATS back-to-back launches after one warm-up launch.  A half-sweep is counted
as sum_r deg_r 2 k^2 + n_rows k^3 / 3 flop (the rank-deg update and the Cholesky factor of every row; the padding to
32 T and the upper-triangle tiles the kernel also computes are not counted) next to the chip's fp64 matrix peak
(78.6 Tflop/s, AMD's MI355X data sheet).  Prints one JSON line per (shape, k).
"""
import argparse
import json
import os
import subprocess
import sys
import time

FIT_REPEATS = 5
KERNEL_REPEATS = 20
FP64_MATRIX_PEAK = 78.6e12


def worker(opts):
    import numpy as np
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from hassaku_amd import hip_ops
    from hassaku_amd.algorithms.base_classes import csr_transpose
    from hassaku_amd.algorithms.mf_algs import AlternatingLeastSquare
    from hassaku_amd.data.csr import UserItemCsr
    from hassaku_amd.data.synthetic import generate, generate_named

    torch.cuda.set_device(0)

    def now():
        torch.cuda.synchronize()
        return time.perf_counter()

    def timed(fn):
        fn()
        t0 = now()
        for _ in range(KERNEL_REPEATS):
            fn()
        return (now() - t0) / KERNEL_REPEATS

    d = generate(3000, 1500, 150000, seed=3) if opts.shape == 's1500' else generate_named(opts.shape, seed=0)
    train = UserItemCsr.from_pairs(d.train[:, 0], d.train[:, 1], d.n_users, d.n_items)
    n_users, n_items, nnz, k = d.n_users, d.n_items, int(train.nnz), opts.k
    alpha, reg = 40.0, 0.01
    model = AlternatingLeastSquare(alpha, k, reg, opts.n_iterations)
    model.fit(train)                       # warm-up
    fits = []
    for _ in range(FIT_REPEATS):
        t0 = now()
        model.fit(train)
        fits.append(now() - t0)

    # the four launches of one iteration, each on its own, on the fitted factors
    dev = model.device
    x_ptr, x_idx = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (train.indptr, train.indices))
    t_ptr, t_idx, _ = csr_transpose(x_ptr, x_idx, None, n_users, n_items)
    X, Xt = (x_ptr, x_idx, n_items), (t_ptr, t_idx, n_users)
    deg_u, deg_i = np.diff(train.indptr), np.bincount(train.indices, minlength=n_items)
    u_order = torch.from_numpy(np.argsort(-deg_u, kind='stable').astype(np.int32)).to(dev)
    i_order = torch.from_numpy(np.argsort(-deg_i, kind='stable').astype(np.int32)).to(dev)
    U, V = model.users_factors, model.items_factors
    out_u, out_v = hip_ops.svd_empty(n_users, k, dev), hip_ops.svd_empty(n_items, k, dev)
    ws = torch.empty(max(hip_ops.svd_gram_ws_bytes(n_users, k), hip_ops.svd_gram_ws_bytes(n_items, k), 16) // 8,
                     dtype=torch.float64, device=dev)
    status = hip_ops.new_status(dev)
    Gv, Gu = hip_ops.svd_gram(V, ws=ws), hip_ops.svd_gram(U, ws=ws)
    t_gram_v = timed(lambda: hip_ops.svd_gram(V, ws=ws))
    t_gram_u = timed(lambda: hip_ops.svd_gram(U, ws=ws))
    t_users = timed(lambda: hip_ops.als_solve(X, V, Gv, alpha, reg, order=u_order, out=out_u, status=status))
    t_items = timed(lambda: hip_ops.als_solve(Xt, U, Gu, alpha, reg, order=i_order, out=out_v, status=status))
    t_users_plain = timed(lambda: hip_ops.als_solve(X, V, Gv, alpha, reg, out=out_u, status=status))
    t_items_plain = timed(lambda: hip_ops.als_solve(Xt, U, Gu, alpha, reg, out=out_v, status=status))
    assert int(status.item()) == 0
    flop_u = float(nnz) * 2 * k * k + n_users * k ** 3 / 3
    flop_i = float(nnz) * 2 * k * k + n_items * k ** 3 / 3
    out = {'shape': opts.shape, 'factors': k, 'n_iterations': opts.n_iterations, 'n_users': n_users,
           'n_items': n_items, 'nnz_train': nnz, 'max_deg_user': int(deg_u.max()), 'max_deg_item': int(deg_i.max()),
           'fit_s': float(np.median(fits)), 'fit_min_s': min(fits), 'fit_max_s': max(fits),
           'gram_items_s': t_gram_v, 'gram_users_s': t_gram_u, 'solve_users_s': t_users, 'solve_items_s': t_items,
           'solve_users_unordered_s': t_users_plain, 'solve_items_unordered_s': t_items_plain,
           'solve_users_peak_fraction': flop_u / t_users / FP64_MATRIX_PEAK,
           'solve_items_peak_fraction': flop_i / t_items / FP64_MATRIX_PEAK, 'fp64_matrix_peak_flops': FP64_MATRIX_PEAK}
    print(json.dumps({key: (round(v, 6) if isinstance(v, float) and abs(v) > 1e-3 else v) for key, v in out.items()}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='s1500,ml1m')
    ap.add_argument('--factors', default='64,128')
    ap.add_argument('--n-iterations', type=int, default=4)
    ap.add_argument('--step-timeout', type=int, default=600, help='seconds each (shape, k) may take')
    ap.add_argument('--shape', help=argparse.SUPPRESS)         # set by the driver: time this one case in this process
    ap.add_argument('--k', type=int, help=argparse.SUPPRESS)
    opts = ap.parse_args()
    if opts.shape:
        worker(opts)
        return 0
    for shape in opts.shapes.split(','):
        for k in opts.factors.split(','):
            cmd = ['timeout', '-k', '10', str(opts.step_timeout), sys.executable, os.path.abspath(__file__),
                   '--shape', shape, '--k', k, '--n-iterations', str(opts.n_iterations)]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                print(f'{shape} k {k}: exit status {rc}; nothing more is started', file=sys.stderr)
                return rc
    return 0


if __name__ == '__main__':
    sys.exit(main())
