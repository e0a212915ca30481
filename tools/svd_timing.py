#!/usr/bin/env python3
"""Wall-clock timing of the SVD model on the HIP device at the synthetic ml1m shape (6040 x 3706, 1 M interactions, of
which the train split is fitted; n_factors = 100): one whole fit with its iteration count, each kernel of an iteration
on its own (both sparse products, the Gram, the right-multiplication, the residuals), the full-catalogue scoring plus
top-100, and scipy.sparse.linalg.svds in float64 on the host's CPUs.

    python tools/svd_timing.py [--shapes ml1m] [--n-factors 100] [--no-cpu] [--step-timeout 900]

Each shape runs in a fresh child process under its own `timeout`; a shape that fails ends the run.  At most 16 host
threads are used.  Each phase is bracketed by torch.cuda.synchronize(); one warm-up fit precedes the timed ones and
`fit_s` is the median of five fits.  A kernel's time is the mean of KERNEL_REPEATS back-to-back launches after one
warm-up launch.  The sparse products move nnz x b x 8 bytes of gathered rows (served from L2: the block is a few MB)
and do nnz x b additions; `spmm_*_gbs` is that gather traffic over the time.  The Gram and the product are counted as
2 n b^2 flop next to the chip's fp64 matrix peak (78.6 Tflop/s, AMD's MI355X data sheet).  `fit_beats_svds` is the
condition the model is held to.  Prints one JSON line per shape.
"""
import argparse
import json
import os
import subprocess
import sys
import time

MAX_THREADS = 16
FIT_REPEATS = 5
KERNEL_REPEATS = 20
FP64_MATRIX_PEAK = 78.6e12


def _threads() -> int:
    return min(MAX_THREADS, int(os.environ.get('OMP_NUM_THREADS') or MAX_THREADS))


def worker(opts):
    import numpy as np
    import scipy.sparse as sp
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from hassaku_amd import hip_ops
    from hassaku_amd.algorithms.base_classes import csr_transpose
    from hassaku_amd.algorithms.mf_algs import SVDAlgorithm
    from hassaku_amd.data.csr import UserItemCsr
    from hassaku_amd.data.synthetic import generate_named

    torch.set_num_threads(_threads())
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

    d = generate_named(opts.shape, seed=0)
    train = UserItemCsr.from_pairs(d.train[:, 0], d.train[:, 1], d.n_users, d.n_items)
    n_users, n, nnz, k = d.n_users, d.n_items, int(train.nnz), opts.n_factors
    model = SVDAlgorithm(k)
    model.fit(train)                       # warm-up (and the model the eval timing uses)
    fits = []
    for _ in range(FIT_REPEATS):
        t0 = now()
        model.fit(train)
        fits.append(now() - t0)
    fit_total = float(np.median(fits))
    b = model.block_width(n_users, n)

    # full-catalogue scoring with the train items at -inf, then top-100
    dev = model.device
    ep, ei = train.to_device(dev)
    chunk = max(1, min(n_users, (1 << 29) // (8 * n)))
    buf = torch.empty((chunk, n), dtype=torch.float64, device=dev)
    score = topk = 0.
    for lo in range(0, n_users, chunk):
        u = torch.arange(lo, min(lo + chunk, n_users), device=dev)
        t0 = now()
        s = model.score_rows(u, excl=(ep, ei), out=buf[:len(u)])
        t1 = now()
        hip_ops.knn_topk_rows(s, 100)
        t2 = now()
        score += t1 - t0
        topk += t2 - t1
    model.check_indices()
    del buf

    # the kernels of one iteration, each on its own
    x_ptr, x_idx = (torch.from_numpy(a).to(dev) for a in (train.indptr, train.indices))
    t_ptr, t_idx, _ = csr_transpose(x_ptr, x_idx, None, n_users, n)
    X, Xt = (x_ptr, x_idx, n), (t_ptr, t_idx, n_users)
    gen = torch.Generator(device=dev).manual_seed(0)
    V, Y, Z = hip_ops.svd_empty(n, b, dev), hip_ops.svd_empty(n, b, dev), hip_ops.svd_empty(n_users, b, dev)
    V.copy_(torch.randn((n, b), dtype=torch.float64, device=dev, generator=gen))
    Q = hip_ops.svd_empty(b, b, dev)
    Q.copy_(torch.randn((b, b), dtype=torch.float64, device=dev, generator=gen))
    out_b = hip_ops.svd_empty(n, b, dev)
    theta = torch.ones(b, dtype=torch.float64, device=dev)
    ws = torch.empty(max(hip_ops.svd_gram_ws_bytes(n_users, b), hip_ops.svd_gram_ws_bytes(n, b)) // 8,
                     dtype=torch.float64, device=dev)
    t_xv = timed(lambda: hip_ops.svd_spmm(X, V, out=Z))
    t_xtz = timed(lambda: hip_ops.svd_spmm(Xt, Z, out=Y))
    t_gram_u = timed(lambda: hip_ops.svd_gram(Z, ws=ws))
    t_gram_i = timed(lambda: hip_ops.svd_gram(Y, ws=ws))
    t_mul = timed(lambda: hip_ops.svd_mul(Y, Q, out=out_b))
    t_res = timed(lambda: hip_ops.svd_residuals(Y, V, theta))
    out = {'shape': opts.shape, 'n_factors': k, 'block': b, 'n_users': n_users, 'n_items': n, 'nnz_train': nnz,
           'fit_s': fit_total, 'fit_min_s': min(fits), 'fit_max_s': max(fits), 'n_iter': model.n_iter_,
           'residual': model.residual_, 'spmm_xv_s': t_xv, 'spmm_xtz_s': t_xtz,
           'spmm_xv_gbs': nnz * b * 8 / t_xv / 1e9, 'spmm_xtz_gbs': nnz * b * 8 / t_xtz / 1e9,
           'gram_users_s': t_gram_u, 'gram_items_s': t_gram_i, 'mul_s': t_mul, 'residuals_s': t_res,
           'gram_users_fp64_flops': 2 * n_users * b * b / t_gram_u, 'mul_fp64_flops': 2 * n * b * b / t_mul,
           'fp64_matrix_peak_flops': FP64_MATRIX_PEAK, 'score_s': score, 'topk_s': topk, 'eval_chunk': chunk}
    if not opts.no_cpu:
        Xs = sp.csr_matrix((np.ones(nnz), train.indices, train.indptr), shape=(n_users, n))
        print(f'{opts.shape}: device steps done, timing svds on the host', file=sys.stderr, flush=True)
        from scipy.sparse.linalg import svds
        t0 = time.perf_counter()
        _, s_ref, _ = svds(Xs, k=k)
        out['scipy_svds_s'] = time.perf_counter() - t0
        out['host_threads'] = _threads()
        out['fit_beats_svds'] = bool(fit_total < out['scipy_svds_s'])
        out['sv_max_rel_diff'] = float(np.abs(np.sort(s_ref)[::-1] / model.singular_values - 1).max())
    print(json.dumps({key: (round(v, 6) if isinstance(v, float) and abs(v) > 1e-3 else v) for key, v in out.items()}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='ml1m')
    ap.add_argument('--n-factors', type=int, default=100)
    ap.add_argument('--no-cpu', action='store_true', help='skip scipy.sparse.linalg.svds on the host')
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
               '--shape', shape, '--n-factors', str(opts.n_factors)] + (['--no-cpu'] if opts.no_cpu else [])
        rc = subprocess.run(cmd, env=env).returncode
        if rc != 0:
            print(f'{shape}: exit status {rc}; nothing more is started', file=sys.stderr)
            return rc
    return 0


if __name__ == '__main__':
    sys.exit(main())
