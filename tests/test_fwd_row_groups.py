"""The forward kernels weigh the rows of a buffer in one pass (hsk_weigh_rows): the scores of the R rows of a buffer sit
in lanes j .. j+R-1 of one vector and the sigmoid is evaluated once for the buffer.  What can go wrong is a buffer that
is not full and the 64-row chunk boundaries of a unit's list, and the sampler cannot force those.  Hand-built batches
go through BprMfFusedState.step(u_idx, i_idx) -- k_prep_external and the same forward as the sampled paths -- and
oracle.MfOracleTrainer replays them over 3 steps.

The negatives of positive b are chosen so that the number falling into partition 0 cycles through 0-8, 62-67, 70-73,
126-130 and 134-136; the rest go to the last partition (P = 4: partitions 1 and 2 take counts of the same cycle first).
A unit's list length then takes every remainder mod 2R (R = 3 and 4), 0 and 1, 63 / 64 / 65, 127 / 128 / 129 and N
itself -- asserted below on the batches themselves.  Tolerances are those of test_step_paths_vs_oracle.py: loss 1e-6
relative, parameters by assert_adam_param_close, exp_avg / exp_avg_sq 1e-5 of the tensor's largest."""
import numpy as np
import pytest

from conftest import assert_adam_param_close, max_norm_err
from test_hip_parity import _fused_state, dev

pytestmark = pytest.mark.gpu

STEPS = 3
N_NEG = 136
COUNTS = list(range(0, 9)) + list(range(62, 68)) + list(range(70, 74)) + list(range(126, 131)) + list(range(134, 137))
LENGTHS = set(range(0, 9)) | {63, 64, 65, 127, 128, 129, N_NEG}   # 0..7: every remainder mod 6 and mod 8

# forward, users, items, D, B, N, expected P, loss
CASES = [
    ('p2', 700, 8000, 256, 2048, N_NEG, 2, 'bpr'),
    ('p2', 700, 8000, 256, 2048, N_NEG, 2, 'bce'),
    ('p4', 1500, 10677, 512, 2048, N_NEG, 4, 'bpr'),    # the headline instantiation
    ('p1', 700, 2000, 256, 2048, N_NEG, 1, 'bpr'),      # k_fwd_ugrad
    ('p1', 700, 2000, 256, 2048, N_NEG, 1, 'bce'),
    ('small', 600, 3706, 402, 128, 50, 1, 'bpr'),       # one workgroup per positive (hsk_fwd_small.h)
]


@pytest.fixture(scope='module')
def ops():
    from hassaku_amd import hip_ops
    return hip_ops


def _bounds(n_items, n_part):
    """partition q = items [ceil(q I / P), ceil((q + 1) I / P))"""
    return [-(-q * n_items // n_part) for q in range(n_part + 1)]


def _batch(rng, step, U, I, B, N, n_part):
    """(u [B], i [B, 1 + N], per-(positive, partition) counts [B, P]); the columns of a row are shuffled, so a unit's
    negatives are scattered over the row's 64-column groups."""
    u = rng.randint(0, U, size=B).astype(np.int64)
    i = np.empty((B, N + 1), dtype=np.int64)
    i[:, 0] = rng.randint(0, I, size=B)
    bnd = _bounds(I, n_part)
    cnt = np.zeros((B, n_part), dtype=np.int64)
    nc = len(COUNTS)
    for b in range(B):
        left = N
        if n_part > 1:
            cnt[b, 0] = min(left, COUNTS[(b + step) % nc])
            left -= cnt[b, 0]
            for q, (mul, add) in zip(range(1, n_part - 1), ((7, 3), (11, 5))):
                cnt[b, q] = min(left, COUNTS[(b * mul + add + step) % nc])
                left -= cnt[b, q]
        cnt[b, n_part - 1] = left
        neg = np.concatenate([rng.randint(bnd[q], bnd[q + 1], size=cnt[b, q]) for q in range(n_part)])
        i[b, 1:] = neg[rng.permutation(N)]
    return u, i, cnt


@pytest.mark.parametrize('fwd,U,I,D,B,N,P,loss', CASES, ids=[f'{c[0]}-d{c[3]}-{c[7]}' for c in CASES])
def test_partial_buffers_and_chunk_boundaries_vs_oracle(ops, oracle, fwd, U, I, D, B, N, P, loss):
    rng = np.random.RandomState(sum(map(ord, fwd + loss)))
    params = {'user_emb': (rng.randn(U, D) * 0.05).astype(np.float32), 'item_emb': (rng.randn(I, D) * 0.05).astype(np.float32),
              'item_bias': (rng.randn(I) * 0.1).astype(np.float32)}
    lr, wd = 1e-3, 1e-4
    batches = [_batch(rng, s, U, I, B, N, P) for s in range(STEPS)]
    if P > 1:
        bnd = _bounds(I, P)
        for u, i, cnt in batches:   # the counts are what the kernel's partition test will find
            for q in range(P):
                assert np.array_equal(((i[:, 1:] >= bnd[q]) & (i[:, 1:] < bnd[q + 1])).sum(axis=1), cnt[:, q])
        seen = set(np.unique(np.concatenate([cnt.reshape(-1) for _, _, cnt in batches])).tolist())
        assert LENGTHS <= seen, sorted(LENGTHS - seen)

    st, t = _fused_state(ops, params, lr, wd, B, N + 1, loss=loss)
    assert st.batch_columns(B, N + 1) == N + P, ('partitions', fwd)
    tr = oracle.MfOracleTrainer(params['user_emb'], params['item_emb'], params['item_bias'], lr=lr, wd=wd, loss=loss)
    for s, (u, i, _) in enumerate(batches):
        st.step(dev(u), dev(i))
        got, ref = st.last_loss(), tr.step(u, i)[0]
        print(f'{fwd}-{loss} step {s}: loss {got!r} oracle {ref!r} rel {abs(got - ref) / abs(ref):.2e}', flush=True)
        assert abs(got - ref) <= 1e-6 * abs(ref), ('loss of step', s, got, ref)
    st.flush()
    st.check_status()
    fig = {k: (max_norm_err(st.m[k].cpu().numpy().reshape(-1), tr.M[k].reshape(-1)),
               max_norm_err(st.v[k].cpu().numpy().reshape(-1), tr.V[k].reshape(-1)),
               max_norm_err(t[k].cpu().numpy().reshape(-1), tr.P[k].reshape(-1))) for k in params}
    print(f'{fwd}-{loss}: ' + ' '.join(f'{k}: m {a:.2e} v {b:.2e} p {c:.2e}' for k, (a, b, c) in fig.items()), flush=True)
    for k in params:
        assert fig[k][0] < 1e-5, ('exp_avg', k, fig[k][0])
        assert fig[k][1] < 1e-5, ('exp_avg_sq', k, fig[k][1])
    for k in params:
        assert_adam_param_close(t[k].cpu().numpy(), tr.P[k], (fwd, loss, k))
