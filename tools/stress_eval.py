#!/usr/bin/env python3
"""Randomised cross-check of the evaluation paths (run on a GPU box: python tools/stress_eval.py [seconds] [seed]).
For random shapes (rows, users, items, D, k, item range, exclusions, biases) and every arithmetic form:
  * fused top-k (no score matrix) == materialised top-k, values / ids / order, bit for bit;
  * materialised scores against float64 within 4e-6 of the largest score;
  * in 30 % of the cases: the item range handed over as a physical shard (item_shard=True) gives the same top-k;
  * in 35 % of the cases either table's rows carry log-uniform scales over 2^+-12, and in every case each score is also held
    to its own scale: |got - ref| / (sum_k |u_k||i_k| + |biases|) of forms 1 and 2 within max(4 x the exact-fp32 form's, 5e-7)
    (the componentwise measure of tests/test_eval_structured.py, where the bound is derived);
  * in 25 % of the cases the tables are the integer / tie constructions of tests/eval_cases.py (rising, falling, saw-toothed, quantised,
    all-equal scores, the best items excluded, ...): every form and path must then return the exact numpy expectation.
one_case(rng) runs one case and returns (ok, desc); draw_case(rng) makes all of a case's random draws without touching the
GPU, so the cases a seed produces can be listed on any machine.  tests/test_stress_slices.py runs fixed slices of this.
(The draws and the order of the forms changed when one_case() was split off: seeds of earlier by-hand runs give other cases.)
Prints one line per case that fails and a summary; exit code 1 on any failure."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from hassaku_amd import hip_ops as ops  # noqa: E402
from conftest import csr_from_pairs  # noqa: E402
import eval_cases as structured  # noqa: E402

DIMS = [4, 8, 16, 30, 32, 36, 64, 100, 128, 200, 256, 402, 512]   # 30: rows not 16-byte aligned -> scalar staging, form 1
REL_FLOOR = 5e-7


def draw_case(rng):
    """All random draws of one case (numpy only).  -> dict: the shape in 'desc', exclusion pairs, the seed of the tables."""
    n_users = int(rng.randint(1, 900))
    n_items = int(rng.choice([rng.randint(1, 300), rng.randint(300, 5000), rng.randint(5000, 60000)]))
    D = int(rng.choice(DIMS))
    R = int(rng.randint(1, 700))
    lo = int(rng.randint(0, n_items)) if rng.rand() < 0.5 else 0
    cnt = int(rng.randint(1, n_items - lo + 1))
    k = int(min(cnt, rng.choice([1, 5, 10, 50, 100, 128])))
    scale = float(10.0 ** rng.uniform(-4, 2))
    table_seed = int(rng.randint(1 << 30))
    ties = bool(n_items > 40 and rng.rand() < 0.5)
    with_ib, with_ub, with_gb = bool(rng.rand() < 0.7), bool(rng.rand() < 0.3), bool(rng.rand() < 0.3)
    pairs = None
    if rng.rand() < 0.7:
        # (drawn sparsely: a dense n_users x n_items draw was 430 MB of host memory for the widest cases)
        dens = min(0.5, float(rng.choice([5.0, 50.0, 300.0])) / n_items)
        flat = np.unique(rng.randint(0, n_users * n_items, size=int(rng.binomial(n_users * n_items, dens))))
        pairs = np.stack([flat // n_items, flat % n_items], axis=1) if len(flat) else None
    u = rng.randint(0, n_users, size=R).astype(np.int64)
    shard = bool(rng.rand() < 0.3)
    row_scales = str(rng.choice(['none', 'none', 'none', 'users', 'items', 'both'], p=[0.25, 0.2, 0.2, 0.1, 0.1, 0.15]))
    su = np.exp2(rng.uniform(-12, 12, size=(n_users, 1))).astype(np.float32)
    si = np.exp2(rng.uniform(-12, 12, size=(n_items, 1))).astype(np.float32)
    integer = None
    if rng.rand() < 0.25:       # the exact constructions: their own tables, biases and exclusions
        kind, hard = structured.B_KINDS[int(rng.randint(len(structured.B_KINDS)))]
        integer = dict(kind=kind, hard=bool(hard), seed=int(rng.randint(1 << 20)))
        n_users = max(n_users, 4)
    desc = dict(shard=shard, n_users=n_users, n_items=n_items, D=D, R=R, lo=lo, cnt=cnt, k=k, scale=scale, Ib=with_ib, Ub=with_ub,
                gb=with_gb, excl=pairs is not None, ties=ties, row_scales=row_scales, integer=integer)
    return dict(desc=desc, pairs=pairs, u=u, table_seed=table_seed, su=su, si=si)


def _tables(c):
    """Device tensors of a drawn case: U, I, Ib, Ub, gb, u, exclusion CSR, and the exact expectation (integer cases)."""
    d = c['desc']
    if d['integer'] is not None:
        g = d['integer']
        s = structured.selection_case((d['R'], d['n_users'], d['n_items'], d['D'], d['k'], None), g['kind'], g['hard'], d['lo'],
                                      d['cnt'], seed=g['seed'])
        expect = structured.expected_topk(s['S'], s['pairs'], s['u'], d['k'], d['lo'])
        t = [None if s[n] is None else torch.from_numpy(s[n]).cuda() for n in ('U', 'I', 'Ib', 'Ub', 'gb', 'u')]
        pairs = s['pairs']
    else:
        g = torch.Generator(device='cuda').manual_seed(c['table_seed'])
        scale, n_users, n_items, D = d['scale'], d['n_users'], d['n_items'], d['D']
        U = torch.randn(n_users, D, device='cuda', generator=g) * scale
        I = torch.randn(n_items, D, device='cuda', generator=g) * scale
        if d['ties']:
            I[n_items // 2: n_items // 2 + 10] = I[:10]          # exact ties
        Ib = (torch.randn(n_items, device='cuda', generator=g) * scale * scale) if d['Ib'] else None
        Ub = (torch.randn(n_users, device='cuda', generator=g) * scale * scale) if d['Ub'] else None
        gb = torch.tensor([0.1 * scale * scale], device='cuda') if d['gb'] else None
        if d['row_scales'] in ('users', 'both'):
            U = U * torch.from_numpy(c['su']).cuda()
        if d['row_scales'] in ('items', 'both'):
            I = I * torch.from_numpy(c['si']).cuda()
        t = [U, I, Ib, Ub, gb, torch.from_numpy(c['u']).cuda()]
        pairs, expect = c['pairs'], None
    e_ptr = e_idx = None
    if pairs is not None:
        p, i = csr_from_pairs(pairs, d['n_users'])
        e_ptr, e_idx = torch.from_numpy(p).cuda(), torch.from_numpy(i).cuda()
    return t, e_ptr, e_idx, expect


def one_case(rng):
    """One random case through every arithmetic form.  -> (ok, desc); desc['fail'] lists what went wrong."""
    c = draw_case(rng)
    what = c['desc']
    lo, cnt, k, R, n_items = what['lo'], what['cnt'], what['k'], what['R'], what['n_items']
    (U, I, Ib, Ub, gb, u), e_ptr, e_idx, expect = _tables(c)
    ref = U[u].double() @ I[lo:lo + cnt].double().T
    den = U[u].double().abs() @ I[lo:lo + cnt].double().abs().T
    for b in ((None if Ub is None else Ub[u].double()[:, None]), (None if Ib is None else Ib[lo:lo + cnt].double()[None, :]),
              (None if gb is None else gb.double())):
        if b is not None:
            ref += b
            den += b.abs()
    fails, rel = [], {}
    try:
        for form in (ops.EVAL_ARITH_FP32, ops.EVAL_ARITH_BF16X3, ops.EVAL_ARITH_F16X2):
            ops.set_eval_arith(form)
            v0, i0, sc = ops.mf_eval_topk(U, I, Ib, Ub, gb, u, k, e_ptr, e_idx, item_begin=lo, item_count=cnt, want_scores=True)
            v1, i1, _ = ops.mf_eval_topk(U, I, Ib, Ub, gb, u, k, e_ptr, e_idx, item_begin=lo, item_count=cnt, want_scores=False)
            ok = torch.equal(v0.view(torch.int32), v1.view(torch.int32)) and torch.equal(i0, i1)
            if what['shard']:   # the same range handed over as a PHYSICAL shard (the library gets a virtual base and must never
                # read outside the shard's rows): same top-k, materialised and fused
                Is, Ibs = I[lo:lo + cnt].contiguous(), (None if Ib is None else Ib[lo:lo + cnt].contiguous())
                for want in (True, False):
                    v2, i2, _ = ops.mf_eval_topk(U, Is, Ibs, Ub, gb, u, k, e_ptr, e_idx, item_begin=lo, item_count=cnt,
                                                 item_shard=True, n_items_global=n_items, want_scores=want)
                    ok = ok and torch.equal(v0.view(torch.int32), v2.view(torch.int32)) and torch.equal(i0, i2)
            got = sc[:R * cnt].view(R, cnt).double()
            fin = torch.isfinite(got)
            err = ((got - ref)[fin].abs().max().item() if fin.any() else 0.0)
            big = max(ref.abs().max().item(), 1e-30)
            ok_acc = err <= 4e-6 * big
            # each score against its own scale; a zero denominator (zero rows, D-wide cancellation cannot make one) wants a zero
            zero = fin & (den == 0)
            ok_zero = bool((got[zero] == 0).all())
            m = fin & (den > 0)
            rel[form] = ((got - ref)[m].abs() / den[m]).max().item() if m.any() else 0.0
            ok_rel = form == ops.EVAL_ARITH_FP32 or rel[form] <= max(4.0 * rel[ops.EVAL_ARITH_FP32], REL_FLOOR)
            ok_exact = True
            if expect is not None:
                ev, ei = expect
                for v, i in ((v0, i0), (v1, i1)):
                    ok_exact = ok_exact and np.array_equal(i.cpu().numpy(), ei) and \
                        np.array_equal(structured.bits(v.cpu().numpy()), structured.bits(ev))
            if not (ok and ok_acc and ok_zero and ok_rel and ok_exact):
                fails.append(dict(form=form, paths_equal=ok, err_over_max=err / big, zero_den_ok=ok_zero, rel=rel[form],
                                  rel_fp32=rel[ops.EVAL_ARITH_FP32], exact=ok_exact))
    finally:
        ops.set_eval_arith(ops.EVAL_ARITH_DEFAULT)
    desc = dict(what, rel={f: float(f'{x:.3g}') for f, x in rel.items()}, fail=fails)
    return not fails, desc


def main():
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    rng = np.random.RandomState(seed)
    t_end = time.time() + budget
    n_case = n_fail = 0
    while time.time() < t_end:
        ok, desc = one_case(rng)
        n_case += 1
        if not ok:
            n_fail += 1
            print('FAIL', desc, flush=True)
    print(f'{n_case} cases, {n_fail} failures', flush=True)
    sys.exit(1 if n_fail else 0)


if __name__ == '__main__':
    main()
