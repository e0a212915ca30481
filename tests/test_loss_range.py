"""The three training losses over the whole score range, against the float64 restatement of tests/loss_restate.py.

Every other training test uses tables at initialisation scale: no argument of a loss leaves [-1, 1], the sigmoid is
0.5 +- 0.1, the online softmax rescales by 0.99 and expf never saturates.  Here the scores run over +-104 and over the
orders in which a running max can move, on inputs ("dial tables", loss_restate.dial_tables) whose scores are EXACT in
fp32 in any summation order -- so what is compared is the loss arithmetic, not the order of a dot product.

Families of a batch (a rule for the columns of a row; build_batch):
  mid    dials of positives and negatives within +-12: nothing saturates, the sigmoid is nonlinear
  wide   dials over +-104: x = s_0 - s (bce: s) falls into every band of BANDS
  ramp   a row's negatives in rising score order: the running max of the online softmax moves at almost every row
  fall   ... in falling order: the max never moves after the first negative
  spike  quiet negatives (dial within +-2) and one of dial +104 at column 1, 64, 65 or N, cycling over b: the rescale
         factor exp(old max - new max) underflows (below 2^-126: zero or one of the last denormals) and what was
         accumulated so far has to vanish
  ties   every negative is the positive's own item: x = 0 exactly, the softmax is uniform up to log_adjust
Every batch but `ties` carries min(B, I // 3) items that occur ONCE in the batch, one in every column 1 .. N across
the rows: the item_bias gradient of such an item is that entry's d loss / d score alone.  (I = 2000 has fewer than
B = 2048 items, hence the min; in `ties` an item fills its whole row.)

The fused step is asked for ONE AdamW step with wd = 0: exp_avg = w1 * g with w1 = float32(1 - beta1), so
st.m[k] / w1 is the gradient the kernels computed, to one more rounding.  The parameters are only held to be finite:
Adam's division amplifies last-bit differences where |g| ~ eps, and a dial input is full of such elements.

The bound.  u = 2^-24 is the relative error of one correctly rounded fp32 operation.  An element of a gradient is
  sum over its entries e of  g_e * operand_e,    g_e = d loss / d s_e,
and it is held to   |got - f64| <= u * (sum_e c_e |g_e| |operand_e|  +  n * sum_e |g_e| |operand_e|):
  * c_e counts the roundings that go into the WEIGHT of entry e before it is used:
      bpr negative / any bce entry   g = inv / (1 + expf(x)):  expf 2 (the device library documents 1 ulp = 2 u),
                                     the add 1, the IEEE division 1, the rounding of inv = 1/(B N) 1, the
                                     multiplication by w1 1, and 2 spare (FMA or not, the sign): C_ENTRY = 8,
                                     i.e. 2^-21 on an element with a single entry -- the per-term bound the evaluation
                                     tests use;
      bpr positive                   g_0 = -gsum, an fp32 sum of the N negative weights (all of one sign) in up to
                                     8 shares (P partitions, 4 / 8 waves, the ranks): C_ENTRY + N + 8;
      sampled softmax                g_k = expf(z_k - M) * (inv / L): C_ENTRY for expf, multiplication, division, inv
                                     and w1, plus the normaliser L, an fp32 sum of N + 1 exponentials (2 each): 2 +
                                     (N + 1); the online form also multiplies what it has accumulated by
                                     f = expf(old max - new max) whenever the max moves (expf 2, the product 1), so term
                                     k of L carries 3 * (moves after k): weighted by its share p_k of L that adds
                                     3 * sum_k p_k moves_after(k) -- computed from the float64 z of the row;
      sampled softmax positive       g_0 = p_0 / B - 1 / B = -(sum of the negatives' exponentials) * (inv / L): the
                                     kernels keep that sum on its own, so there is no difference of nearly equal
                                     numbers where p_0 -> 1 and g_0 is held to its OWN magnitude like every entry;
                                     the negatives' sum adds 2 + N and 3 per later move weighted by the term's share
                                     of it.  (Formed as expf(s_0 - M) * (inv / L) - inv, the reference's fp32 form, the
                                     weight missed this bound wherever p_0 came within 2^-24 of 1.)
  * n counts the fp32 additions of the element's own sum, one u of sum |terms| each whatever the order: the
    occurrences of item i in the batch less one for item_emb / item_bias (an item that occurs once is held to
    8 * 2^-24 = 2^-21); for a user row, per occurrence of the user, the N + 1 terms of the axpy chain plus 8 for the
    partial rows of P partitions or of 4 / 8 waves, less one.
An element whose float64 value times w1 is below 2^-126 (fp32 subnormal) is held to the same count of 2^-149 steps
instead (the larger of the two bounds), and an element whose scale is zero has to be exactly zero.  The bound is
derived, not measured: the measured worst cases are printed in the ROW lines and recorded in MEASUREMENTS.md.

The un-fused operators (ops.bpr_loss_grad, ops.rec_loss_grad) get explicit logits on the same ladder, every entry of
the returned gradient held to u * c_e * |g_e| (no sum, no moments).  The sharded step is run on two ranks with
N = 2, so that a rank holds none of a positive's negatives for about half of the positives (its running max stays
-inf and k_shard_ssm_fix merges 0 * expf(-inf - M)).
"""
import functools
import os

import numpy as np
import pytest

import loss_restate as lr
from conftest import max_norm_err

ADJ = 2.75                      # a dyadic log_adjust: z = s + ADJ stays exact in fp32 (log(I / N) would round it once)
U24 = 2.0 ** -24
W1 = float(np.float32(1.0 - 0.9))   # the library's lerp weight (float)(1.0 - beta1)
C_ENTRY = 8
SUM_SHARES = 8
FAMILIES = ('mid', 'wide', 'ramp', 'fall', 'spike', 'ties')
BANDS = ('<-88.8', '[-88.8,-20)', '[-20,-1)', '[-1,1]', '(1,20]', '(20,88.8]', '>88.8')
PROMISED = {'mid': (2, 3, 4), 'wide': tuple(range(7)), 'ramp': tuple(range(7)), 'fall': tuple(range(7)),
            'spike': (0, 2, 3, 4), 'ties': (3,)}

# forward, users, items, D, B, N, expected P, losses, losses that also run ramp / fall / spike / ties
FORWARDS = [
    ('part_p2', 700, 8000, 256, 2048, 136, 2, ('bpr', 'bce'), ()),
    ('part_p4', 1500, 10677, 512, 2048, 136, 4, ('bpr',), ()),
    ('ugrad_large', 700, 2000, 256, 2048, 136, 1, ('bpr', 'bce', 'sampled_softmax'), ('bpr', 'sampled_softmax')),
    ('wg_8waves', 600, 3706, 402, 128, 50, 1, ('bpr', 'bce'), ()),
    ('wg_4waves', 600, 3706, 402, 128, 9, 1, ('bpr',), ()),
    ('ugrad_small_early', 600, 3706, 64, 128, 70, 1, ('sampled_softmax',), ('sampled_softmax',)),
    ('ugrad_small_late', 600, 3706, 402, 128, 70, 1, ('sampled_softmax',), ('sampled_softmax',)),
]
FUSED_CASES = [(f[0], loss, fam) for f in FORWARDS for loss in f[7]
               for fam in FAMILIES if fam in ('mid', 'wide') or loss in f[8]]
_FWD = {f[0]: f for f in FORWARDS}
CPU_SHAPE = ('cpu', 60, 200, 24, 32, 70)     # the restatement's own checks: crosses the 64-row chunk too


def _seed(*words):
    return sum((k + 1) * ord(ch) for k, ch in enumerate('/'.join(map(str, words)))) % (2 ** 31)


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=3)
def tables(U, I, D, dial_max=None):
    """dial tables of a shape, the items' classes and the float64 score matrix -- computed once per shape"""
    P, cls = lr.dial_tables(np.random.RandomState(_seed('tables', U, I, D)), U, I, D, dial_max)
    return P, cls, lr.score_matrix(P)


def band_counts(x):
    x = np.asarray(x).reshape(-1)
    return np.array([(x < -88.8).sum(), ((x >= -88.8) & (x < -20)).sum(), ((x >= -20) & (x < -1)).sum(),
                     ((x >= -1) & (x <= 1)).sum(), ((x > 1) & (x <= 20)).sum(), ((x > 20) & (x <= 88.8)).sum(),
                     (x > 88.8).sum()])


def spike_column(b, N):
    return (1, min(64, N), min(65, N), N)[b % 4]


def n_solo_items(B, I):
    return min(B, I // 3)


def build_batch(cls, S, B, N, family, rng):
    """(u [B], i [B, 1 + N]) int64 by the family's rule; S is the float64 [users, items] score matrix."""
    U, I = S.shape
    quiet, midc, spike, floor = (cls == k for k in (0, 1, 3, 4))
    pool = {'mid': quiet | midc, 'spike': quiet}.get(family, np.ones(I, bool))
    u = rng.randint(0, U, size=B).astype(np.int64)
    i = np.empty((B, N + 1), dtype=np.int64)
    if family == 'ties':
        i[:] = rng.choice(np.flatnonzero(pool), size=B)[:, None]
        return u, i
    n_solo = n_solo_items(B, I)
    cand = rng.permutation(np.flatnonzero(pool & ~spike & ~floor))
    solo, rest = cand[:n_solo], np.setdiff1d(np.flatnonzero(pool), cand[:n_solo])
    assert len(solo) == n_solo and len(rest) >= 8, (family, len(solo), len(rest))
    i[:, 0] = rng.choice(rest, size=B)
    i[:, 1:] = rng.choice(rest, size=(B, N))
    col = 1 + (np.arange(B) + np.arange(B) // N) % N   # the column of row b's once-only item (the shift per cycle
    #                                                    keeps it from meeting the spike's column, b % 4, every time)
    if family in ('ramp', 'fall'):
        # row b: col - 1 negatives that score below its once-only item, N - col above, sorted by score; the once-only
        # items go to the rows in the order of their dials so that both sides have items to draw from
        rows = np.argsort(col[:n_solo], kind='stable')
        solo_of = np.empty(n_solo, dtype=np.int64)
        solo_of[rows] = solo[np.argsort(S[0, solo], kind='stable')]
        for b in range(B):
            sc = S[u[b]]
            if b < n_solo:
                lo, hi = rest[sc[rest] < sc[solo_of[b]]], rest[sc[rest] > sc[solo_of[b]]]
                neg = np.concatenate([rng.choice(lo, size=col[b] - 1), [solo_of[b]], rng.choice(hi, size=N - col[b])])
            else:
                neg = i[b, 1:]
            i[b, 1:] = neg[np.argsort(sc[neg], kind='stable')]
        if family == 'fall':
            i[:, 1:] = i[:, :0:-1].copy()
        return u, i
    if family == 'spike':
        for b in range(B):
            sp_col = spike_column(b, N)
            i[b, sp_col] = rng.choice(np.flatnonzero(spike))
            if col[b] == sp_col:
                col[b] = col[b] % N + 1
    i[np.arange(n_solo), col[:n_solo]] = solo
    return u, i


def running_max_moves(z):
    """z float64 [B, K] -> bool [B, K]: entry k > 0 raises the running max that starts at z_0"""
    before = np.maximum.accumulate(z, axis=1)[:, :-1]
    return np.concatenate([np.zeros((len(z), 1), bool), z[:, 1:] > before], axis=1)


def check_batch(S, u, i, loss, family, what=''):
    """What a batch promises, asserted on the host before any launch.  -> float64 scores [B, K]"""
    B, K = i.shape
    N = K - 1
    s = S[u[:, None], i]
    z = s.copy()
    if loss == 'sampled_softmax':
        z[:, 1:] += ADJ
    x = s[:, :1] - s[:, 1:]
    for name, a in (('s', s), ('x', x), ('z', z)):     # exact in fp32: scores, differences, adjusted scores
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a), (what, name)
        assert np.array_equal(a * 256, np.round(a * 256)) and np.abs(a).max() < 512, (what, name)
    bands = band_counts(s if loss == 'bce' else x)
    assert all(bands[k] > 0 for k in PROMISED[family]), (what, dict(zip(BANDS, bands)))
    moves = running_max_moves(z)
    if family == 'ramp':
        assert moves.sum(axis=1).max() >= N / 2, (what, moves.sum(axis=1).max())
    if family == 'fall':
        assert not moves[:, 2:].any(), what
    if family == 'spike':
        cols = np.array([spike_column(b, N) for b in range(B)])
        before = np.array([z[b, :c].max() for b, c in enumerate(cols)])
        assert set(cols) == {1, min(64, N), min(65, N), N}, what
        assert (np.exp(before - z[np.arange(B), cols]) < 2.0 ** -126).all(), what
        assert (z[np.arange(B), cols] == z.max(axis=1)).all(), what
    if family == 'ties':
        assert (x == 0).all() and (i == i[:, :1]).all(), what
    else:
        occ = np.bincount(i.reshape(-1), minlength=S.shape[1])
        once = occ[i] == 1
        assert len(np.unique(i[once])) >= n_solo_items(B, S.shape[1]), (what, once.sum())
        assert once[:, 1:].any(axis=0).all(), (what, 'a column without a once-only item')
    return s


def fused_case(fwd, loss, family):
    """-> (P, S, u, i, expected partitions)"""
    _, U, I, D, B, N, n_part, _, _ = _FWD[fwd]
    P, cls, S = tables(U, I, D)
    u, i = build_batch(cls, S, B, N, family, np.random.RandomState(_seed(fwd, loss, family)))
    return P, S, u, i, n_part


# ------------------------------------------------------------------------------------------------
# the bound
# ------------------------------------------------------------------------------------------------
def entry_bounds(ref, loss, online, abs_e=0.0):
    """float64 [B, K]: the error allowed on the weight of each entry, c_e * u * magnitude_e + abs_e (module docstring)"""
    g = ref['g']
    B, K = g.shape
    c = np.full(g.shape, float(C_ENTRY))
    mag = np.abs(g)
    if loss == 'bpr':
        c[:, 0] += (K - 1) + SUM_SHARES
    elif loss == 'sampled_softmax':
        p, z = ref['aux']['p'], ref['aux']['z']
        norm, negs = np.full(B, 2.0 + K), np.full(B, 2.0 + (K - 1))   # the normaliser L; the negatives' own sum
        if online:
            moves = running_max_moves(z)
            after = moves.sum(axis=1, keepdims=True) - np.cumsum(moves, axis=1)
            norm += 3.0 * (p * after).sum(axis=1)
            negs += 3.0 * (p[:, 1:] * after[:, 1:]).sum(axis=1) / p[:, 1:].sum(axis=1)
        c += norm[:, None]
        c[:, 0] += negs
    return c * U24 * mag + abs_e


def grad_bounds(P, u, i, ref, loss, online=True, abs_e=0.0, w1=W1):
    """{name: per-element bound on |got - f64|} for the three dense gradients (module docstring)"""
    Ue, Ie = np.abs(P['user_emb'].astype(np.float64)), np.abs(P['item_emb'].astype(np.float64))
    K = i.shape[1]
    weighted = dict(zip(('user_emb', 'item_emb', 'item_bias'),
                        lr.dense_products(Ue, Ie, u, i, entry_bounds(ref, loss, online, abs_e))))
    n_user = np.maximum(np.bincount(u, minlength=len(Ue)) * (K + SUM_SHARES) - 1, 0)    # additions: terms - 1
    n_item = np.maximum(np.bincount(i.reshape(-1), minlength=len(Ie)) - 1, 0)
    terms = {'user_emb': n_user[:, None], 'item_emb': n_item[:, None], 'item_bias': n_item}
    out = {}
    for k, t in weighted.items():
        scale = ref['scale'][k]
        tol = t + U24 * terms[k] * scale
        tiny = (np.abs(ref['grads'][k]) * w1 < 2.0 ** -126) & (scale > 0)
        steps = np.divide(tol, U24 * scale, out=np.zeros_like(tol), where=scale > 0)    # the element's count c
        out[k] = np.where(tiny, np.maximum(tol, steps * 2.0 ** -149 / w1), tol)
    return out


def compare(got, val, scale, tol, w1):
    """Figures of one tensor: over the elements with scale * w1 >= 2^-126, the worst |err| / scale and the bound / scale at
    that element; over those below (every term subnormal in the moment), the worst |err| and its bound in steps of
    2^-149; the worst |err| / bound of all; the number of elements with a zero scale that are not exactly zero."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - val)
    has = scale > 0
    safe = np.where(has, scale, 1.0)
    tiny = has & (scale * w1 < 2.0 ** -126)
    rel = np.where(has & ~tiny, err / safe, 0.0).reshape(-1)
    k = int(np.argmax(rel))
    steps = np.where(tiny, err, 0.0).reshape(-1) * w1 / 2.0 ** -149
    j = int(np.argmax(steps))
    return {'rel': float(rel[k]), 'rel_bound': float((tol / safe).reshape(-1)[k]), 'steps': float(steps[j]),
            'steps_bound': float(tol.reshape(-1)[j] * w1 / 2.0 ** -149) if tiny.any() else 0.0,
            'ratio': float(np.where(has, err / np.where(has, tol, 1.0), 0.0).max()),
            'nonzero': int(((~has) & (got != 0)).sum())}


def grad_figures(got, P, u, i, ref, loss, what, online=True, abs_e=0.0, w1=W1):
    """got: {name: float array} -> {name: compare(...)}, one ROW line printed per tensor"""
    tol = grad_bounds(P, u, i, ref, loss, online, abs_e, w1)
    figs = {k: compare(got[k], ref['grads'][k], ref['scale'][k], tol[k], w1) for k in ('item_bias', 'item_emb', 'user_emb')}
    for k, f in figs.items():
        print(f'ROW {what} {k}: worst err/scale {f["rel"]:.2e} (bound there {f["rel_bound"]:.2e}); subnormal: worst err '
              f'{f["steps"]:.2f} steps of 2^-149 (bound there {f["steps_bound"]:.1f}); worst err/bound {f["ratio"]:.3f}; '
              f'nonzero at zero scale {f["nonzero"]}', flush=True)
    return figs


def assert_figures(figs, what):
    for k, f in figs.items():
        assert f['nonzero'] == 0, (what, k, 'elements with a zero scale that are not exactly zero', f['nonzero'])
        assert f['ratio'] <= 1.0, (what, k, 'error / bound', f)


def assert_grads(got, P, u, i, ref, loss, what, **kw):
    assert_figures(grad_figures(got, P, u, i, ref, loss, what, **kw), what)


# ------------------------------------------------------------------------------------------------
# without a GPU: the restatement itself, and every batch the GPU tests use
# ------------------------------------------------------------------------------------------------
def _cpu_inputs(kind):
    _, U, I, D, B, N = CPU_SHAPE
    if kind == 'dial':
        P, cls, S = tables(U, I, D)
        u, i = build_batch(cls, S, B, N, 'wide', np.random.RandomState(5))
        return P, S, u, i
    rng = np.random.RandomState(6)
    P = lr.init_tables(rng, U, I, D)
    return P, lr.score_matrix(P), rng.randint(0, U, size=B).astype(np.int64), rng.randint(0, I, size=(B, N + 1)).astype(np.int64)


@pytest.mark.parametrize('loss', lr.LOSSES)
@pytest.mark.parametrize('kind', ['init', 'dial'])
def test_restatement_vs_float64_autograd(kind, loss):
    """the textbook expressions in torch float64 with autograd through a [B, K, D] gather"""
    import torch
    import torch.nn.functional as F
    P, S, u, i = _cpu_inputs(kind)
    ref = lr.restate(P, u, i, loss, ADJ, S)
    t = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in P.items()}
    ut, it = torch.from_numpy(u), torch.from_numpy(i)
    s = (t['user_emb'][ut][:, None, :] * t['item_emb'][it]).sum(-1) + t['item_bias'][it]
    if loss == 'bpr':
        val = -F.logsigmoid(s[:, :1] - s[:, 1:]).mean()
    elif loss == 'bce':
        y = torch.zeros_like(s)
        y[:, 0] = 1.0
        val = F.binary_cross_entropy_with_logits(s.flatten(), y.flatten())
    else:
        z = torch.cat([s[:, :1], s[:, 1:] + ADJ], dim=1)
        val = (-z[:, 0] + torch.logsumexp(z, dim=1)).mean()
    val.backward()
    assert abs(ref['loss'] - val.item()) <= 1e-13 * abs(val.item()), (ref['loss'], val.item())
    assert np.abs(ref['scores'] - s.detach().numpy()).max() <= 1e-12
    # autograd's softmax - 1 and sigmoid - 1 cancel in float64: 2^-50 of the entry's normalisation
    inv = np.abs(ref['g']).sum(axis=1).max()
    slack = dict(zip(('user_emb', 'item_emb', 'item_bias'),
                     lr.dense_products(np.abs(P['user_emb'].astype(np.float64)), np.abs(P['item_emb'].astype(np.float64)),
                                       u, i, np.full(i.shape, 2.0 ** -50 * inv))))
    for k in slack:
        err = np.abs(ref['grads'][k] - t[k].grad.numpy())
        assert (err <= 1e-12 * ref['scale'][k] + slack[k]).all(), (k, err.max())


@pytest.mark.parametrize('loss', lr.LOSSES)
@pytest.mark.parametrize('kind', ['init', 'dial'])
def test_restatement_vs_oracle_step_one(oracle, kind, loss):
    """oracle.MfOracleTrainer: fp32 scores (exact on a dial input; on an initialisation-scale input the restatement is
    given the oracle's own rounded scores), weights evaluated in double and cast to fp32, fp32 sums in the reference's
    order -- inside the bound of the module docstring plus the 2^-50 of the oracle's (sigmoid - 1) and (softmax - 1)."""
    P, S, u, i = _cpu_inputs(kind)
    tr = oracle.MfOracleTrainer(P['user_emb'], P['item_emb'], P['item_bias'], lr=1e-3, wd=0.0, loss=loss, log_adjust=ADJ)
    val, logits, g, grads = tr.step(u, i)
    exact = lr.batch_scores(P, u, i, S)
    if kind == 'dial':
        assert np.array_equal(logits.astype(np.float64), exact)
    else:
        assert np.abs(logits - exact).max() < 1e-6
    ref = lr.restate(P, u, i, loss, ADJ, scores=logits.astype(np.float64))
    # (the oracle rounds x = s_0 - s to fp32 like the reference: exact on a dial input, 2^-24 |x| otherwise)
    assert abs(val - ref['loss']) <= (1e-12 if kind == 'dial' else 1e-8) * abs(ref['loss']), (val, ref['loss'])
    inv = np.abs(ref['g']).sum(axis=1).max()
    slack = 2.0 ** -50 * inv + 2.0 ** -149     # ... and the cast of a subnormal weight to fp32
    assert (np.abs(g - ref['g']) <= entry_bounds(ref, loss, False, slack)).all()
    assert_grads(grads, P, u, i, ref, loss, f'oracle-{kind}-{loss}', online=False, abs_e=slack, w1=1.0)
    for k in grads:        # and the first moments are w1 * g, which is how the GPU tests read the gradients
        if grads[k] is not None:
            assert max_norm_err(tr.M[k] / W1, grads[k]) < 2 * U24, k


@pytest.mark.parametrize('shape', sorted({f[1:4] for f in FORWARDS} | {CPU_SHAPE[1:4]}))
def test_dial_scores_are_exact_in_fp32(shape):
    """the fp32 BLAS product and a sequential fp32 accumulation (with the bias added last, and first) both equal the
    float64 scores element for element; the noise stays small beside the dial"""
    P, cls, S = tables(*shape)
    Ue, Ie, Ib = P['user_emb'], P['item_emb'], P['item_bias']
    assert np.array_equal((Ue @ Ie.T + Ib).astype(np.float64), S)
    rows = slice(0, 48)
    for first in (False, True):
        acc = np.tile(Ib, (48, 1)) if first else np.zeros((48, len(Ib)), np.float32)
        for d in range(shape[2]):
            acc += Ue[rows, d:d + 1] * Ie[:, d]
        assert acc.dtype == np.float32 and np.array_equal((acc if first else acc + Ib).astype(np.float64), S[rows])
    dial = Ie[:, -1].astype(np.float64)
    assert np.array_equal(dial * 16, np.round(dial * 16)) and np.abs(dial).max() == lr.DIAL_SPIKE
    assert (Ue[:, -1] == 1).all() and (S - dial).std() < 0.5
    assert all((cls == k).sum() >= 4 for k in range(len(lr.CLASSES)))


@pytest.mark.parametrize('fwd,loss,family', FUSED_CASES, ids=['-'.join(c) for c in FUSED_CASES])
def test_fused_batches_keep_their_promises(fwd, loss, family):
    """the host-side assertions of every batch the GPU tests launch: exact scores, bands, moves, once-only items"""
    P, S, u, i, _ = fused_case(fwd, loss, family)
    check_batch(S, u, i, loss, family, (fwd, loss, family))


# ------------------------------------------------------------------------------------------------
# the fused step
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def ops():
    from hassaku_amd import hip_ops
    return hip_ops


@pytest.mark.gpu
@pytest.mark.parametrize('fwd,loss,family', FUSED_CASES, ids=['-'.join(c) for c in FUSED_CASES])
def test_fused_step_gradients_over_the_score_range(ops, fwd, loss, family):
    """One step of every forward on every family it is asked for.  (`wide` at the small batches is the regression test
    of hsk_sigmoid_neg_scaled: inv / (1 + expf(x)) alone is 0 from x = 88.72 on, where inv * exp(-x) is still an fp32
    subnormal -- 2.8 to 18 times the subnormal bound at B * N = 6400 and 1152; MEASUREMENTS.md.)"""
    from test_hip_parity import _fused_state, dev
    P, S, u, i, n_part = fused_case(fwd, loss, family)
    B, K = i.shape
    what = f'{fwd}-{loss}-{family}'
    check_batch(S, u, i, loss, family, what)
    ref = lr.restate(P, u, i, loss, ADJ, S)

    st, t = _fused_state(ops, P, 1e-3, 0.0, B, K, loss=loss, log_adjust=ADJ if loss == 'sampled_softmax' else 0.0,
                         optimizer='adamw')
    assert st.batch_columns(B, K) == K - 1 + n_part, ('partitions', fwd)
    st.step(dev(u), dev(i))
    got_loss = st.last_loss()
    st.flush()
    st.check_status()
    print(f'ROW {what} loss: got {got_loss!r} f64 {ref["loss"]!r} rel {abs(got_loss - ref["loss"]) / abs(ref["loss"]):.2e}',
          flush=True)
    m = {k: st.m[k].cpu().numpy().astype(np.float64).reshape(P[k].shape) for k in P}
    finite = {k: bool(np.isfinite(t[k].cpu().numpy()).all() and np.isfinite(m[k]).all()
                      and np.isfinite(st.v[k].cpu().numpy()).all()) for k in P}
    print(f'ROW {what} finite: {finite}', flush=True)
    figs = grad_figures({k: m[k] / W1 for k in m}, P, u, i, ref, loss, what)     # every figure is out before the first assert
    assert all(finite.values()), (what, finite)
    assert abs(got_loss - ref['loss']) <= 1e-6 * abs(ref['loss']), (what, got_loss, ref['loss'])
    assert_figures(figs, what)


# ------------------------------------------------------------------------------------------------
# the un-fused operators on explicit logits
# ------------------------------------------------------------------------------------------------
OPS_B = 64
OPS_N = (1, 63, 64, 65, 136)


def ladder_logits(loss, family, N, rng):
    """float64 [OPS_B, 1 + N], multiples of 1/16 within +-104 (the sampled softmax's negatives within +-100, so that
    z = logit + ADJ stays exact in fp32), by the family's rule"""
    top = 100.0 if loss == 'sampled_softmax' else 104.0
    bound = {'mid': 12.0, 'spike': 2.0}.get(family, 104.0)
    s = np.empty((OPS_B, N + 1))
    s[:, 0] = lr._sixteenths(rng, OPS_B, min(bound, top))
    s[:, 1:] = lr._sixteenths(rng, (OPS_B, N), min(bound, top))
    if family == 'ramp':
        s[:, 1:] = np.sort(s[:, 1:], axis=1)
    elif family == 'fall':
        s[:, 1:] = np.sort(s[:, 1:], axis=1)[:, ::-1]
    elif family == 'spike':
        for b in range(OPS_B):
            s[b, spike_column(b, N)] = top
    elif family == 'ties':
        s[:, 1:] = s[:, :1]
    return s


@pytest.mark.gpu
@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('loss', lr.LOSSES)
def test_loss_operators_on_ladder_logits(ops, loss, family):
    from test_hip_parity import dev
    rows = []
    for N in OPS_N:
        s = ladder_logits(loss, family, N, np.random.RandomState(_seed('ops', loss, family, N)))
        s32 = s.astype(np.float32)
        assert np.array_equal(s32.astype(np.float64), s)
        z = s + np.concatenate([[0.0], np.full(N, ADJ if loss == 'sampled_softmax' else 0.0)])
        assert np.array_equal(z.astype(np.float32).astype(np.float64), z)
        if family == 'wide' and N >= 63:
            assert (band_counts(s if loss == 'bce' else s[:, :1] - s[:, 1:]) > 0).all()
        val, g, aux = lr.loss_and_entry_grads(s, loss, ADJ)
        ref = {'g': g, 'aux': aux}
        if loss == 'bpr':
            got_loss, got = ops.bpr_loss_grad(dev(s32))
        else:
            got_loss, got = ops.rec_loss_grad(loss, dev(s32), ADJ)
        got_loss, got = float(got_loss.item()), got.cpu().numpy().astype(np.float64)
        tol = entry_bounds(ref, loss, online=False)
        steps = tol / np.where(g != 0, U24 * np.abs(g), 1.0)
        tol = np.where(np.abs(g) < 2.0 ** -126, np.maximum(tol, steps * 2.0 ** -149), tol)
        err = np.abs(got - g)
        rel = float((err / np.where(g != 0, np.abs(g), 1.0)).max())
        rows.append((N, got_loss, val, bool(np.isfinite(got).all()), float((err / tol).max()), rel))
        print(f'ROW ops-{loss}-{family} N={N}: loss {got_loss!r} f64 {val!r} rel {abs(got_loss - val) / abs(val):.2e} '
              f'worst err/|g| {rel:.2e} worst err/bound {rows[-1][4]:.3f}', flush=True)
    for N, got_loss, val, finite, ratio, rel in rows:
        assert finite, (loss, family, N)
        assert abs(got_loss - val) <= 1e-6 * abs(val), (loss, family, N, got_loss, val)
        assert ratio <= 1.0, (loss, family, N, 'error / bound', ratio, 'worst error / |g|', rel)


# ------------------------------------------------------------------------------------------------
# the sharded step: a rank that holds none of a positive's negatives
# ------------------------------------------------------------------------------------------------
SHARD = dict(D=64, U=211, I=300, B=48, N=2, world=2, seed=77, dial_max=40.0)


def _shard_problem():
    P, _, S = tables(SHARD['U'], SHARD['I'], SHARD['D'], SHARD['dial_max'])
    rng = np.random.RandomState(3)
    pairs = np.argwhere(rng.rand(SHARD['U'], SHARD['I']) < 0.06)
    return P, S, pairs[rng.permutation(len(pairs))]


def _range_shard_worker(rank, world, port, out_dir, loss):
    import torch
    import torch.distributed as dist
    from conftest import csr_from_pairs
    from test_dist import _dev, _init
    _init(rank, world, port, 'gloo')
    torch.cuda.set_device(0)
    from hassaku_amd.dist import Comm, ShardedBprMf
    comm = Comm()
    P, _, pairs = _shard_problem()
    ptr, idx = csr_from_pairs(pairs, SHARD['U'])
    t = {k: _dev(v) for k, v in P.items()}
    sh = ShardedBprMf(comm, t['user_emb'], t['item_emb'], t['item_bias'], None, None, lr=1e-3, wd=0.0, batch=SHARD['B'],
                      n_neg=SHARD['N'], csr_indptr=_dev(ptr), csr_indices=_dev(idx), coo_user=_dev(pairs[:, 0], torch.int32),
                      coo_item=_dev(pairs[:, 1], torch.int32), seed=SHARD['seed'], native='host-staged', loss=loss,
                      log_adjust=ADJ if loss == 'sampled_softmax' else 0.0)
    assert sh.issued_natively and sh.backend() == 'host-staged'
    order = torch.from_numpy(np.random.RandomState(1).permutation(len(pairs))).cuda()
    sh.step_sampled(order, 0, next_start=None)
    val = sh.last_loss()
    sh.check_status()
    offs, items, ug = (x.cpu().numpy() for x in sh.last_batch())
    m, v = sh.gather_item_moments()
    full_u, _ = sh.gather_user_table()
    full_i, full_ib = sh.gather_item_table()
    np.savez(os.path.join(out_dir, f'kept{rank}.npz'), offs=offs, items=items, ug=ug, lo=sh.item_lo, hi=sh.item_hi)
    if rank == 0:
        np.savez(os.path.join(out_dir, 'out.npz'), loss=val, m=m.cpu().numpy(), v=v.cpu().numpy(), U=full_u.cpu().numpy(),
                 I=full_i.cpu().numpy(), Ib=full_ib.cpu().numpy())
    sh.close()
    dist.destroy_process_group()


def _global_batch(ops, loss):
    """the global batch of the sharded step's first step: the single-GPU fused step with the same seed, order and step
    numbering draws the same samples (test_dist._single_gpu_reference)"""
    import torch
    from conftest import csr_from_pairs
    from test_dist import _dev
    P, _, pairs = _shard_problem()
    ptr, idx = csr_from_pairs(pairs, SHARD['U'])
    t = {k: _dev(v) for k, v in P.items()}
    G, N = SHARD['world'] * SHARD['B'], SHARD['N']
    st = ops.BprMfFusedState(t['user_emb'], t['item_emb'], t['item_bias'], None, None, lr=1e-3, wd=0.0, max_batch=G,
                             max_cols=N + 1, seed=SHARD['seed'], csr_indptr=_dev(ptr), csr_indices=_dev(idx),
                             coo_user=_dev(pairs[:, 0], torch.int32), coo_item=_dev(pairs[:, 1], torch.int32), loss=loss,
                             log_adjust=ADJ if loss == 'sampled_softmax' else 0.0)
    order = torch.from_numpy(np.random.RandomState(1).permutation(len(pairs))).cuda()
    st.step_sampled(order, 0, G, N)
    st.flush()
    st.check_status()
    bu, bi = st.last_batch(G, N + 1)
    return bu.cpu().numpy().astype(np.int64), bi.cpu().numpy().astype(np.int64)


def test_shard_tables_are_dial_tables():
    P, S, pairs = _shard_problem()
    assert np.abs(P['item_emb'][:, -1]).max() <= SHARD['dial_max'] and len(pairs) >= SHARD['world'] * SHARD['B']
    assert np.array_equal(S.astype(np.float32).astype(np.float64), S)
    assert np.array_equal((S + ADJ).astype(np.float32).astype(np.float64), S + ADJ)
    assert np.array_equal((P['user_emb'] @ P['item_emb'].T + P['item_bias']).astype(np.float64), S)


@pytest.mark.gpu
@pytest.mark.parametrize('loss', ['sampled_softmax', 'bpr'])
def test_sharded_step_with_ranks_that_hold_no_negative(ops, tmp_path, loss):
    import torch.multiprocessing as mp
    from test_dist import _free_port
    world, G, N = SHARD['world'], SHARD['world'] * SHARD['B'], SHARD['N']
    mp.spawn(_range_shard_worker, args=(world, _free_port(), str(tmp_path), loss), nprocs=world, join=True)
    r = np.load(os.path.join(str(tmp_path), 'out.npz'))
    P, S, _ = _shard_problem()
    u, i = _global_batch(ops, loss)
    empty = 0
    for rank in range(world):      # each rank kept exactly the global batch's entries inside its item range
        k = np.load(os.path.join(str(tmp_path), f'kept{rank}.npz'))
        lo, hi = int(k['lo']), int(k['hi'])
        assert np.array_equal(k['ug'], u)
        for b in range(G):
            assert list(k['items'][k['offs'][b]:k['offs'][b + 1]]) == [x - lo for x in i[b] if lo <= x < hi], (rank, b)
        empty += int((~((i[:, 1:] >= lo) & (i[:, 1:] < hi)).any(axis=1)).sum())
    ref = lr.restate(P, u, i, loss, ADJ, S)
    assert np.array_equal(ref['scores'].astype(np.float32).astype(np.float64), ref['scores'])
    got_loss = float(r['loss'])
    err_m = max_norm_err(r['m'].astype(np.float64) / W1, ref['grads']['item_emb'])
    finite = all(bool(np.isfinite(r[k]).all()) for k in ('m', 'v', 'U', 'I', 'Ib'))
    print(f'ROW shard-{loss}: (positive, rank) pairs without a negative {empty} of {world * G}; loss {got_loss!r} f64 '
          f'{ref["loss"]!r} rel {abs(got_loss - ref["loss"]) / abs(ref["loss"]):.2e}; item exp_avg / largest {err_m:.2e}; '
          f'finite {finite}', flush=True)
    assert empty * 4 >= world * G, (empty, world * G)
    assert finite
    assert abs(got_loss - ref['loss']) <= 2e-5 * abs(ref['loss']), (got_loss, ref['loss'])
    assert err_m < 1e-5, err_m
