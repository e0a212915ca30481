#!/usr/bin/env python3
"""Device time of hsk_calibration_metrics at evaluation sizes, next to the reference's torch expressions
(eval/eval.py:170-197 there: gather item_mtx[idx_topk] -> [rows, k, n_bins], sum, smooth, the three distances, for each
of the four cut-offs) run on the same device tensors.

    python tools/calibration_timing.py [--rows 16384] [--items 10677] [--bins 18,3,1000] [--repeats 20]

The default shape is one ml10m evaluation chunk: 16 384 rows x 100 ranked ids, 18 tags and 3 popularity buckets, plus
1000 bins for a wide tag vocabulary.  Per shape and item dtype: the median and the extremes of `repeats` samples
(device events around 50 back-to-back kernel calls, or one pass of the torch expressions; three warm-up calls first),
the bytes the kernel gathers per call (rows x k_max x n_bins x element size) and that figure
over the median time, and what the torch expressions allocate at their peak.  The kernel's and the torch expressions' results are compared on the finite entries
before anything is timed.  Prints one JSON line per shape."""
import argparse
import json
import os
import sys

KS = [100, 50, 10, 5]
WARMUP = 3
KERNEL_CALLS_PER_SAMPLE = 50   # a sample is 50 launches back to back: one launch is tens of microseconds


def torch_expressions(ids, users, item_mtx, user_mtx, beta):
    import torch
    from hassaku_amd.eval.metrics import hellinger_distance, jensen_shannon_distance, kl_divergence
    p = user_mtx[users]
    out = []
    for k in KS:
        q = item_mtx[ids[:, :k]].sum(1)
        q /= k
        q = beta * p + (1 - beta) * q
        out.append(torch.stack([hellinger_distance(p, q), jensen_shannon_distance(p, q), kl_divergence(p, q)], -1))
    return torch.stack(out, 1)


def timed(fn, repeats, inner=1):
    """(median, min, max) seconds per call over `repeats` samples of `inner` back-to-back calls each"""
    import torch
    for _ in range(WARMUP):
        fn()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3 / inner)
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=16384)
    ap.add_argument('--items', type=int, default=10677)
    ap.add_argument('--users', type=int, default=69878)
    ap.add_argument('--bins', default='18,3,1000')
    ap.add_argument('--repeats', type=int, default=20)
    opts = ap.parse_args()
    import numpy as np
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from hassaku_amd import hip_ops
    if not torch.cuda.is_available():
        raise SystemExit('calibration_timing needs a HIP device: a time taken anywhere else says nothing')
    torch.cuda.set_device(0)
    rng = np.random.RandomState(0)
    for n_bins in (int(b) for b in opts.bins.split(',')):
        # items with one to three bins (one-hot for the popularity shape), users smoothed like the builders' rows
        hot = rng.rand(opts.items, n_bins).argsort(1) < (1 if n_bins <= 3 else rng.randint(1, 4, (opts.items, 1)))
        item32 = torch.from_numpy((hot / hot.sum(1, keepdims=True)).astype(np.float32)).cuda()
        user32 = torch.from_numpy((.01 / n_bins + .99 * rng.dirichlet(np.ones(n_bins), opts.users)).astype(np.float32)).cuda()
        user64 = user32.double()
        ids = torch.from_numpy(rng.randint(0, opts.items, (opts.rows, 100)).astype(np.int32)).cuda()
        ids64 = ids.long()
        users = torch.from_numpy(rng.randint(0, opts.users, opts.rows).astype(np.int64)).cuda()
        dev = hip_ops.calibration_metrics(ids, users, item32, user64, .01, KS)
        ref = torch_expressions(ids64, users, item32, user32, .01).double()
        fin = torch.isfinite(ref) & torch.isfinite(dev)
        out = {'rows': opts.rows, 'k_max': 100, 'n_items': opts.items, 'n_bins': n_bins, 'ks': KS,
               'finite_share': round(float(fin.double().mean()), 4),
               'max_abs_diff_vs_torch_fp32': float((dev - ref)[fin].abs().max())}
        del dev, ref
        for name, item in (('fp32', item32), ('fp64', item32.double())):
            med, lo, hi = timed(lambda: hip_ops.calibration_metrics(ids, users, item, user64, .01, KS), opts.repeats,
                                inner=KERNEL_CALLS_PER_SAMPLE)
            gathered = opts.rows * 100 * n_bins * item.element_size()
            out.update({f'kernel_{name}_s': med, f'kernel_{name}_min_s': lo, f'kernel_{name}_max_s': hi,
                        f'gathered_bytes_{name}': gathered, f'gathered_bytes_per_s_{name}': gathered / med})
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        med, lo, hi = timed(lambda: torch_expressions(ids64, users, item32, user32, .01), max(3, opts.repeats // 4))
        out.update({'torch_s': med, 'torch_min_s': lo, 'torch_max_s': hi,
                    'torch_peak_bytes': torch.cuda.max_memory_allocated() - before,
                    'torch_over_kernel_fp32': med / out['kernel_fp32_s']})
        print(json.dumps({k: (float(f'{v:.4g}') if isinstance(v, float) else v) for k, v in out.items()}), flush=True)
        del item32, user32, user64, ids, ids64, users
        torch.cuda.empty_cache()
    return 0


if __name__ == '__main__':
    sys.exit(main())
