"""The ranked half of every evaluation against exact restatements (tests/rank_restate.py): the fp64 selection
(`knn_block_topk` behind hsk_knn_topk_rows and hsk_knn_select), hsk_rank_metrics, and the two device loops of
evaluate_recommender_algorithm with more than one chunk.

Every expectation is computed in numpy.  Selections are held integer for integer and bit for bit; precision and recall bit
for bit to the correctly rounded float32 quotient; ndcg to c * 2^-24 relative with c counted from the kernel's own
roundings (rank_restate.ndcg_c); the loops to their single-call results bit for bit.

ndcg bound.  c(k) = 2 (2 e + 1 + ceil(k / 64) - 1 + 6) + 1 with e the ulp error of log2f.  The toolchain ships no
device-math accuracy table, so e = 2 is an ASSUMPTION: c = 23 for k <= 64, 25 for k <= 128, 53 for k = 1024, i.e.
1.4e-6 .. 3.2e-6 relative.  That is above the 1e-6 the older tests use: theirs is an observed figure, not a worst case (the
roundings of ~10 + ceil(k / 64) operations per sum do not all point one way).  The measured worst |got - f64| / (2^-24 f64)
is printed by test_rank_metrics_cases and recorded in MEASUREMENTS.md."""
import types

import numpy as np
import pytest

import knn_restate as kr
import rank_restate as rr
from conftest import csr_from_pairs, load_golden
from eval_cases import expected_topk, selection_case

U24 = 2.0 ** -24


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _neg(x):
    """-x by the sign bit alone (also for NaN and 0)."""
    return (rr.bits64(x) ^ rr.SIGN).view(np.float64)


def _from_bits(*patterns):
    return np.array(patterns, dtype=np.uint64).view(np.float64)


# =====================================================================================================================
# 1. the restatement itself (CPU)
# =====================================================================================================================
def test_key64_is_the_order_of_doubles():
    rng = np.random.RandomState(0)
    x = rng.randint(0, 2 ** 32, size=4000).astype(np.uint64) << np.uint64(32) | rng.randint(0, 2 ** 32, size=4000).astype(np.uint64)
    x = np.concatenate([_from_bits(1, 2, (1 << 63) | 1, (1 << 52) - 1, 1 << 52), rng.randn(200),
                        [1., -1., np.nextafter(1., 2.), np.nextafter(-1., -2.), 1e308, -1e308], x.view(np.float64)])
    x = x[np.isfinite(x) & (x != 0)][:1500]
    assert len(x) == 1500 and (np.abs(x) < 2.3e-308).any()
    key = rr.key64(x)
    assert key.dtype == np.uint64 and np.array_equal(key[:, None] < key[None, :], x[:, None] < x[None, :])
    # beyond `<`: the pinned places of the values that `<` cannot rank
    special = np.concatenate([_from_bits(0xfff8000000000000), [-np.inf, -1., -5e-324, -0.], [0., 5e-324, 1., np.inf],
                              _from_bits(0x7ff0000000000001, 0x7ff8000000000000)])
    assert np.all(np.diff(rr.key64(special).astype(object)) > 0)


def test_topk64_equals_knn_restate():
    rng = np.random.RandomState(1)
    S = np.round(rng.randn(6, 700) * 4) / 4                     # ties
    S[S == 0] = 0.                                              # no -0.0
    excl = [rng.choice(700, size=m, replace=False) for m in (0, 5, 650, 699, 700, 30)]
    for k in (1, 7, 100, 700):
        v, i = kr.masked_topk(S, excl, k)
        masked = S.copy()
        for q, cols in enumerate(excl):
            masked[q, cols] = -np.inf
        ids, bits = rr.topk64(masked, k)
        assert np.array_equal(ids, i) and np.array_equal(bits, rr.bits64(v))
    valid = np.ones(S.shape, bool)
    for q, cols in enumerate(excl):
        valid[q, cols] = False
    ids, bits = rr.topk64(S, 100, valid)
    for q, cols in enumerate(excl):
        m = min(100, 700 - len(cols))
        assert np.array_equal(ids[q, :m], kr.masked_topk(S[q:q + 1], [cols], 100)[1][0, :m])
        assert (ids[q, m:] == -1).all() and not bits[q, m:].any()


def test_rank_metrics64_equals_golden_and_torch_functions():
    import torch
    from hassaku_amd.eval.metrics import ndcg_at_k_batch, precision_at_k_batch, recall_at_k_batch
    fx = load_golden('g5_metrics.npz')
    y = fx['y_true']
    labels = [np.flatnonzero(row > 0) for row in y]
    ks = [5, 10, 50, 100]
    m = rr.rank_metrics64(fx['top100'], labels, ks)['metrics']
    for t, k in enumerate(ks):
        for j, name in enumerate(('precision', 'recall', 'ndcg')):
            np.testing.assert_allclose(m[:, t, j], fx[f'{name}@{k}'], rtol=1e-5, atol=1e-7, err_msg=f'{name}@{k}')
    # the torch functions on CPU tensors, lists with duplicated ids and users without labels
    rng = np.random.RandomState(2)
    R, I = 40, 300
    yt = (rng.rand(R, I) < .05).astype(np.float32)
    yt[3] = 0
    yt[4, :150] = 1
    ids = rng.randint(0, I, size=(R, 100))
    ids[5, :20] = ids[5, 0]
    yt[5, ids[5, 0]] = 1                                        # a hit that stands at twenty ranks counts twenty times
    ks = [100, 1, 37, 64]
    ref = rr.rank_metrics64(ids, [np.flatnonzero(r) for r in yt], ks)
    for t, k in enumerate(ks):
        top = torch.from_numpy(ids[:, :k])
        p, r, n = (fn(None, torch.from_numpy(yt), k, aggr_sum=False, idx_topk=top).numpy()
                   for fn in (precision_at_k_batch, recall_at_k_batch, ndcg_at_k_batch))
        assert np.array_equal(p, rr.f32_ratio(ref['hits'][:, t], k))
        assert np.array_equal(r, np.where(ref['n_rel'] > 0, rr.f32_ratio(ref['hits'][:, t], np.maximum(ref['n_rel'], 1)), 0))
        # torch: float32 log2, reciprocal, k products and a sum of k terms per DCG / IDCG, one division
        np.testing.assert_allclose(n, ref['metrics'][:, t, 2], rtol=(2 * (k + 4) + 1) * U24, atol=0)
    assert ref['metrics'][3, :, 1:].max() == 0 and ref['hits'][5, 0] >= 20


def test_ndcg_c_stays_what_the_docstring_says():
    assert [rr.ndcg_c(k) for k in (1, 64, 65, 128, 1024)] == [23, 23, 25, 25, 53]


# =====================================================================================================================
# 2. hsk_knn_topk_rows against topk64
# =====================================================================================================================
WIDTHS = [1, 2, 255, 256, 257, 4095, 4096, 4097, 8193, 20481]
FAMILIES = ['spread', 'low_bits', 'classes', 'sorted', 'masked', 'tiny', 'nan']
NAN_BITS = (0x7ff8000000000000, 0xfff8000000000000, 0x7ff0000000000001, 0xffffffffffffffff, 0x7ff8000000000000)


def _cutoffs(n):
    return sorted({1, min(n, 100), min(n, 1024)} | ({n} if n <= 1024 else set()))


def _family(name, n, k, rng):
    """[3..5, n] float64 rows of one value family."""
    j = np.arange(n)
    if name == 'spread':
        return rng.randn(4, n)
    if name == 'low_bits':      # keys that share their upper six bytes: pass after pass until the bucket fits the cap
        return np.stack([1. + rng.permutation(n) * 2. ** -52 for _ in range(3)])
    if name == 'classes':
        hi, mid, lo = 1. + 2 * 2. ** -52, 1. + 2. ** -52, 1.        # distinct in the last byte only
        ragged = n - (n - 1) // 256 * 256                           # width of the last 256-column stripe
        rows = [np.array([hi, mid, lo])[j % 3],                     # the threshold class is the top one, in every stripe
                np.where(j >= n - ragged, hi, np.where(j % 2 == 0, mid, lo)),    # the winners in the last stripe only
                np.where(j % 97 == 5, hi, np.where(j % 4 != 0, mid, lo)),        # few on top, k cuts the middle class
                np.full(n, mid),
                np.array([3., -1., .5])[(j * 7 + 1) % 3]]
        return np.stack(rows)
    if name == 'sorted':
        T = (n + 255) // 256
        return np.stack([j * .5, (n - 1 - j) * .5, ((T - 1 - j // 256) * 256 + j % 256) * .5,
                         ((j // 256) * 256 + 255 - j % 256) * .5])
    if name == 'masked':        # k - 5 finite entries, scattered and at the very end; then none
        m = max(k - 5, 0)
        S = np.full((3, n), -np.inf)
        S[0, rng.choice(n, size=m, replace=False)] = np.round(rng.randn(m) * 2)
        S[1, n - m:] = rng.randn(m)
        return S
    if name == 'tiny':
        pool = np.array([0., -0., 5e-324, -5e-324, 1e-310, -1e-310, 2.2250738585072014e-308, -2.2250738585072014e-308, 1e-320])
        return np.stack([pool[rng.randint(0, len(pool), size=n)], pool[rng.randint(0, 2, size=n)],
                         pool[rng.randint(0, 4, size=n)], rng.randn(n) * 1e-310])
    assert name == 'nan'
    S = np.round(rng.randn(4, n) * 3) / 3
    nans = _from_bits(*NAN_BITS)
    for q in range(2):
        at = rng.choice(n, size=min(n, 5), replace=False)
        S[q, at] = nans[:len(at)]
    S[1, rng.randint(0, n, size=2)] = [np.inf, -np.inf]
    S[2] = nans[0]                                                   # one NaN everywhere: index order
    S[3] = nans[rng.randint(0, len(nans), size=n)]                   # NaNs only, of several patterns
    return S


@pytest.mark.gpu
@pytest.mark.parametrize('n', WIDTHS)
@pytest.mark.parametrize('family', FAMILIES)
def test_topk_rows_families(family, n):
    """ids integer for integer and values bit for bit, every cut-off, the family and its negation, ld = n and ld = n + 3
    with +inf and NaN in the padding columns."""
    import torch
    from hassaku_amd import hip_ops
    rng = np.random.RandomState(n + 7 * len(family))
    pad = np.array([np.inf, np.nan, np.inf])
    for k in _cutoffs(n):
        base = _family(family, n, k, rng)
        for S in (base, _neg(base)):
            ids, bits = rr.topk64(S, k)
            wide = np.concatenate([S, np.tile(pad, (len(S), 1))], 1)
            for dev, n_cols in ((_dev(S), None), (_dev(wide), n)):
                v, i = hip_ops.knn_topk_rows(dev, k, n_cols)
                assert v.shape == i.shape == (len(S), k) and i.dtype == torch.int32 and v.dtype == torch.float64
                got_i, got_v = i.cpu().numpy(), v.cpu().numpy().view(np.uint64)
                bad = np.argwhere(got_i != ids)
                assert not len(bad), (family, n, k, dev.shape[1], 'first wrong (row, slot)', bad[0], got_i[tuple(bad[0])],
                                      ids[tuple(bad[0])])
                assert np.array_equal(got_v, bits), (family, n, k, dev.shape[1])
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_topk_rows_order_of_zeros_and_nans():
    """The convention of DESIGN section 2, pinned: NaN (sign clear) > +inf > ... > +0.0 > -0.0 > ... > -inf > NaN (sign set)."""
    import torch
    from hassaku_amd import hip_ops
    row = np.concatenate([[-0., np.inf, 1.], _from_bits(0xfff8000000000000), [0., -np.inf], _from_bits(0x7ff8000000000000),
                          [-1., 0., -0.]])
    v, i = hip_ops.knn_topk_rows(_dev(row[None, :]), len(row))
    assert i.cpu().numpy().tolist() == [[6, 1, 2, 4, 8, 0, 9, 7, 5, 3]]
    assert np.array_equal(v.cpu().numpy().view(np.uint64)[0], rr.bits64(row[[6, 1, 2, 4, 8, 0, 9, 7, 5, 3]]))
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_topk_rows_refusals_write_nothing():
    import torch
    from hassaku_amd import _lib, hip_ops
    lib = _lib.load()
    S = _dev(np.random.RandomState(0).randn(3, 50))
    for k, n_cols, ld in ((0, 50, 50), (1025, 50, 50), (51, 50, 50), (1025, 2000, 2000), (5, 51, 50), (5, 50, 49)):
        vals = torch.full((3, 1100), 7.25, dtype=torch.float64, device='cuda')
        ids = torch.full((3, 1100), -77, dtype=torch.int32, device='cuda')
        rc = lib.hsk_knn_topk_rows(S.data_ptr(), 3, n_cols, ld, k, vals.data_ptr(), ids.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
        with pytest.raises(RuntimeError, match='hsk_knn_topk_rows'):
            _lib.check(rc, 'hsk_knn_topk_rows')
        torch.cuda.synchronize()
        assert bool((vals == 7.25).all()) and bool((ids == -77).all()), (k, n_cols, ld)
    for k, n_cols in ((0, None), (1025, None), (51, None), (5, 51)):
        with pytest.raises(RuntimeError):
            hip_ops.knn_topk_rows(S, k, n_cols)
    torch.cuda.synchronize()


# =====================================================================================================================
# 3. hsk_knn_select on constructed count blocks
# =====================================================================================================================
SIM_PARAMS = {'cosine': {}, 'jaccard': {}, 'sorensen_dice': {}, 'asymmetric_cosine': {'alpha': .4},
              'tversky': {'alpha': .3, 'beta': .7}}
SEL_GARBAGE = 5                 # columns of the block beyond n


def _small_block(k, rng, n=1300, row0=3):
    """Counts from {1, 2, 3}; rows: no valid column, one, k - 1 / k / k + 1 of them, the own column the best, negative and
    zero counts among positive ones, everything valid."""
    C = np.zeros((8, n), dtype=np.int64)
    own = row0 + np.arange(8)
    C[0, own[0]] = 5
    C[1, 777] = 2
    for r, m in ((2, k - 1), (3, k), (4, k + 1)):
        cols = rng.choice(np.setdiff1d(np.arange(n), [own[r]]), size=m, replace=False)
        C[r, cols] = rng.randint(1, 4, size=m)
        C[r, own[r]] = 3                                     # the own column is never a candidate
    C[5] = rng.randint(1, 3, size=n)
    C[5, own[5]] = 3                                         # ... although it would be the best
    C[6] = rng.randint(-2, 4, size=n)
    C[7] = rng.randint(1, 4, size=n)
    return C, row0


def _wide_block(n=5000, row0=2500):
    """n = 5000: one similarity value with more than 4096 members; k cuts inside it (below 30 better ones, or at the top)."""
    j = np.arange(n)
    C = np.stack([np.where(j % 160 == 9, 3, np.where(j < 4700, 2, 1)), np.where(j >= 350, 3, 1),
                  np.where(j % 2 == 0, 2, np.where(j % 4 == 1, 3, 0))])
    return C.astype(np.int64), row0


@pytest.mark.gpu
@pytest.mark.parametrize('shrinkage', [0., 10.])
@pytest.mark.parametrize('kind', list(SIM_PARAMS))
def test_knn_select_constructed_blocks(kind, shrinkage):
    import torch
    from hassaku_amd import hip_ops
    rng = np.random.RandomState(len(kind) + int(shrinkage))
    a, b = SIM_PARAMS[kind].get('alpha'), SIM_PARAMS[kind].get('beta')
    for k in (1, 100, 1024):
        blocks = [_small_block(k, rng) + ('equal',), _small_block(k, rng) + ('two',), _wide_block() + ('equal',)]
        for C, row0, degrees in blocks:
            rows, n = C.shape
            deg = np.full(n, 9, dtype=np.int64) if degrees == 'equal' else np.where(np.arange(n) % 3 == 0, 4, 9).astype(np.int64)
            own = row0 + np.arange(rows)
            sim = kr.similarity_rows(C, own, deg, kind, shrinkage, a, b)
            valid = (C > 0) & (np.arange(n)[None, :] != own[:, None])
            ids, bits = rr.topk64(sim, k, valid)
            lens = np.minimum(valid.sum(1), k)
            block = np.full((rows, n + SEL_GARBAGE), 7777, dtype=np.int32)      # garbage beyond n: valid if it were read
            block[:, :n] = C
            f64 = lambda x: None if x is None else _dev(np.ascontiguousarray(x, np.float64))    # noqa: E731
            sq = f64(np.sqrt(deg.astype(np.float64))) if kind == 'cosine' else None
            pa = f64(np.power(deg, a)) if kind == 'asymmetric_cosine' else None
            p1a = f64(np.power(deg, 1 - a)) if kind == 'asymmetric_cosine' else None
            oi, ov, ol = hip_ops.knn_select(_dev(block), rows, row0, _dev(deg), sq, pa, p1a, kind, a, b, shrinkage, k)
            what = (kind, shrinkage, k, n, degrees)
            assert np.array_equal(ol.cpu().numpy(), lens), what
            assert np.array_equal(oi.cpu().numpy(), ids), what
            assert np.array_equal(ov.cpu().numpy().view(np.uint64), bits), what
            if n < 4096:
                assert lens[[0, 1, 2, 3, 4, 5, 7]].tolist() == [0, 1, k - 1, k, k, k, k] and 1 <= lens[6] <= k
    torch.cuda.synchronize()


# =====================================================================================================================
# 4. hsk_rank_metrics against rank_metrics64
# =====================================================================================================================
N_ITEMS = 2 ** 31 - 2
K_MAXES = [1, 5, 63, 64, 65, 100, 128, 1024]
_worst_ndcg = {'units': 0., 'of_c': 0.}


def _label_rows(k_max, rng):
    """Users: 0 none, 1 one label, 2 exactly k_max, 3 5000 labels, 4 both ends of the id range, 5 none, 6 5000 labels up to
    the end of the range, 7 none, 8 three labels."""
    big = np.unique(rng.randint(0, N_ITEMS, size=5200))
    big = big[(big < 40000) | (big >= 60000)][:5000]           # (the lists' filler ids live in [40000, 60000))
    top = N_ITEMS - 1 - np.arange(0, 3 * 5000, 3)[::-1]
    rows = [[], [7], 1000 + 3 * np.arange(k_max), big, [0, N_ITEMS - 1], [], top, [], [5, 50, 500]]
    return [np.asarray(r, dtype=np.int64) for r in rows]


def _ks_sets(k_max):
    c = lambda x: int(min(max(x, 1), k_max))        # noqa: E731
    return [[k_max], [c(k_max // 2)], [k_max, 1, c(k_max // 2), c(5), k_max, c(64), c(65), c(63)]]


def _lists(k_max, ks, labels, rng):
    """(user, list, tag) scenarios; the filler ids are even numbers of a range in which no label row has an even id."""
    out = []
    filler = lambda m: 40000 + 2 * rng.permutation(3 * k_max + 8)[:m]     # noqa: E731

    def with_hits(u, at):
        lst = filler(k_max)
        lab = labels[u]
        lst[list(at)] = lab[rng.permutation(len(lab))[:len(at)]]
        return lst

    for u, lab in enumerate(labels):
        m = min(k_max, len(lab))
        out.append((u, with_hits(u, range(m)), 'perfect' if m else 'no labels'))
        out.append((u, filler(k_max), 'no hit'))
    for k in sorted(set(ks)):
        for u in (1, 3, 4, 8):
            out.append((u, with_hits(u, [k - 1]), 'last counted rank'))
            if k < k_max:
                out.append((u, with_hits(u, [k]), 'first rank not counted'))
    out.append((3, np.full(k_max, rr.PAD_ID), 'pads only'))
    out.append((0, np.full(k_max, rr.PAD_ID), 'pads only'))
    lst = np.full(k_max, rr.PAD_ID)
    lst[:min(3, k_max)] = [5, 41000, 500][:min(3, k_max)]
    out.append((8, lst, 'pads after three'))
    lst = filler(k_max)
    lst[:min(3, k_max)] = 7
    out.append((1, lst, 'duplicated hit'))                       # one label, hit up to three times: the clamp at 1
    lst = filler(k_max)
    lst[:min(4, k_max)] = [0, N_ITEMS - 1, 0, N_ITEMS - 1][:min(4, k_max)]
    out.append((4, lst, 'duplicated hit'))
    for u in (3, 6, 2, 8):                                       # a random mixture
        lst = filler(k_max)
        at = np.flatnonzero(rng.rand(k_max) < .3)[:len(labels[u])]
        lst[at] = labels[u][rng.permutation(len(labels[u]))[:len(at)]]
        out.append((u, lst, 'mixed'))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('k_max', K_MAXES)
def test_rank_metrics_cases(k_max):
    import torch
    from hassaku_amd import hip_ops
    rng = np.random.RandomState(k_max)
    labels = _label_rows(k_max, rng)
    assert all(((x < 40000) | (x >= 60000) | (x % 2 == 1)).all() for x in labels) and len(labels[3]) == 5000   # fillers never hit
    lp = np.zeros(len(labels) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in labels], out=lp[1:])
    li = np.concatenate(labels).astype(np.int32)
    lp_d, li_d = _dev(lp), _dev(li)
    for ks in _ks_sets(k_max):
        cases = _lists(k_max, ks, labels, rng)
        order = np.concatenate([np.arange(len(cases)), rng.randint(0, len(cases), size=259)])[:259]
        u = np.array([cases[c][0] for c in order], dtype=np.int64)            # a permutation with repeats
        ids = np.stack([cases[c][1] for c in order]).astype(np.int32)
        tags = [cases[c][2] for c in order]
        assert len(cases) <= 259 and not np.array_equal(u, np.arange(259))
        ref = rr.rank_metrics64(ids, [labels[x] for x in u], ks)
        kk = np.array(ks)
        p_ref = rr.f32_ratio(ref['hits'], kk[None, :])
        r_ref = np.where(ref['n_rel'][:, None] > 0, rr.f32_ratio(ref['hits'], np.maximum(ref['n_rel'], 1)[:, None]),
                         np.float32(0))
        n_ref = ref['metrics'][:, :, 2]
        c = np.array([rr.ndcg_c(k) for k in ks], dtype=np.float64)
        assert (c * U24 < 4e-6).all()
        for n_rows in (1, 4, 5, 259):
            got = hip_ops.rank_metrics(_dev(ids[:n_rows]), _dev(u[:n_rows]), lp_d, li_d, ks)
            assert got.shape == (n_rows, len(ks), 3) and got.dtype == torch.float32
            got = got.cpu().numpy()
            what = (k_max, ks, n_rows)
            assert np.array_equal(got[:, :, 0].view(np.int32), p_ref[:n_rows].view(np.int32)), what
            assert np.array_equal(got[:, :, 1].view(np.int32), r_ref[:n_rows].astype(np.float32).view(np.int32)), what
            err = np.abs(got[:, :, 2].astype(np.float64) - n_ref[:n_rows])
            units = np.where(n_ref[:n_rows] > 0, err / (U24 * np.where(n_ref[:n_rows] > 0, n_ref[:n_rows], 1)), err / U24)
            _worst_ndcg['units'] = max(_worst_ndcg['units'], float(units.max()))
            _worst_ndcg['of_c'] = max(_worst_ndcg['of_c'], float((units / c[None, :]).max()))
            assert (units <= c[None, :]).all(), what + (float(units.max()),)
            for q in range(n_rows):
                if tags[q] in ('perfect', 'duplicated hit'):
                    assert (got[q, :, 2] == np.float32(1)).all(), what + (tags[q], q)
                if tags[q] in ('no labels', 'pads only', 'no hit') or len(labels[u[q]]) == 0:
                    assert not got[q, :, 1:].any(), what + (tags[q], q)
        dup = [q for q in range(259) if tags[q] == 'duplicated hit' and u[q] == 1]
        assert ref['metrics'][dup[0], ks.index(max(ks)), 1] == min(3, max(ks))    # recall is not clamped, ndcg is
    print(f'k_max {k_max}: worst |ndcg - f64| / (2^-24 f64) so far = {_worst_ndcg["units"]:.3f} units, '
          f'{_worst_ndcg["of_c"]:.3f} of c')
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_rank_metrics_refusals_and_foreign_user_id():
    import torch
    from hassaku_amd import hip_ops
    ids = _dev(np.arange(40, dtype=np.int32).reshape(4, 10))
    u = _dev(np.array([1, 0, 1, 0], dtype=np.int64))
    lp, li = _dev(np.array([0, 2, 5], dtype=np.int64)), _dev(np.array([3, 4, 10, 11, 30], dtype=np.int32))
    for ks in ([], list(range(1, 10)), [5, 0], [11], [10, 11]):
        with pytest.raises(RuntimeError, match='hsk_rank_metrics'):
            hip_ops.rank_metrics(ids, u, lp, li, ks)
    # a user id outside the label CSR: no status word here -- the row is scored as user 0's (stated in the header)
    ref = hip_ops.rank_metrics(ids, _dev(np.array([0, 0, 0, 0], dtype=np.int64)), lp, li, [10, 5])
    got = hip_ops.rank_metrics(ids, _dev(np.array([2, 0, -1, 1 << 40], dtype=np.int64)), lp, li, [10, 5])
    assert torch.equal(got, ref)
    torch.cuda.synchronize()


# =====================================================================================================================
# 5. the device loops of evaluate_recommender_algorithm
# =====================================================================================================================
EVAL_KS = [100, 50, 10, 5]       # FullEvaluator.K_VALUES, largest first (the loops' order)
NAMES = ('precision', 'recall', 'ndcg')


def _evaluate(alg, dataset, evaluator, device, batch_size=256):
    """-> (results, (first user, length) of every chunk).  hsk_rank_metrics cannot report a foreign user id (it has no
    status word), so the loops must hand it contiguous arange ids only: checked on every chunk."""
    from hassaku_amd.eval.eval import evaluate_recommender_algorithm
    chunks, inner = [], evaluator.eval_ranked

    def spy(u_idxs, metrics, ks):
        lo = int(u_idxs[0])
        assert np.array_equal(u_idxs.cpu().numpy(), np.arange(lo, lo + len(u_idxs))) and lo + len(u_idxs) <= dataset.n_users
        chunks.append((lo, len(u_idxs)))
        inner(u_idxs, metrics, ks)
    evaluator.eval_ranked = spy
    res = evaluate_recommender_algorithm(alg, types.SimpleNamespace(dataset=dataset, batch_size=batch_size), evaluator, device)
    return res, chunks


def _hold_to_restatement(per_user, ids, label_rows, what):
    """per_user [U, 4, 3] float32 (EVAL_KS order) within the bounds of part 4 of rank_metrics64 on the exact ids."""
    ref = rr.rank_metrics64(ids, label_rows, EVAL_KS)
    kk = np.array(EVAL_KS)
    n_rel = ref['n_rel']
    assert np.array_equal(per_user[:, :, 0], rr.f32_ratio(ref['hits'], kk[None, :])), what
    assert np.array_equal(per_user[:, :, 1], np.where(n_rel[:, None] > 0, rr.f32_ratio(ref['hits'], np.maximum(n_rel, 1)[:, None]),
                                                      np.float32(0))), what
    n_ref = ref['metrics'][:, :, 2]
    c = np.array([rr.ndcg_c(k) for k in EVAL_KS], dtype=np.float64)
    assert (np.abs(per_user[:, :, 2].astype(np.float64) - n_ref) <= c[None, :] * U24 * n_ref).all(), what


def _stack(res, prefix=''):
    return np.stack([np.stack([res[f'{prefix}{name}@{k}'] for name in NAMES], -1) for k in EVAL_KS], 1)


def _hold_groups(run, per_user, groups, what):
    """run(evaluator) -> results.  Per-user results by group, the aggregated means to 1e-12 of the float64 means of the
    per-user float32 values, and the empty group (1 of 3) exactly as FullEvaluator treats it on CPU tensors: per user it
    has keys with empty arrays, aggregated its 0 / 0 raises ZeroDivisionError in get_results()."""
    import torch
    from hassaku_amd.eval.eval import FullEvaluator
    n = len(groups)
    assert set(np.unique(groups)) == {0, 2}
    g3 = torch.from_numpy(groups)
    met_cpu = torch.from_numpy(per_user)
    # per user, three groups
    res = run(FullEvaluator(False, 3, g3))
    cpu = FullEvaluator(False, 3, g3)
    cpu.eval_ranked(torch.arange(n), met_cpu, EVAL_KS)
    cpu_res = cpu.get_results()
    assert sorted(res) == sorted(cpu_res) and len(res) == 48, what
    for name in res:
        assert res[name].dtype == np.float32 and np.array_equal(res[name], cpu_res[name]), (what, name)
    assert all(res[f'group_1_{m}@{k}'].shape == (0,) for m in NAMES for k in EVAL_KS)
    # aggregated, one group empty: the same refusal as on CPU tensors, with the sums of the other groups in place
    cpu = FullEvaluator(True, 3, g3)
    cpu.eval_ranked(torch.arange(n), met_cpu, EVAL_KS)
    with pytest.raises(ZeroDivisionError):
        cpu.get_results()
    ev = FullEvaluator(True, 3, g3)
    with pytest.raises(ZeroDivisionError):
        run(ev)
    assert int(ev.n_entries[1]) == 0 and all(float(v) == 0. for v in ev.group_metrics[1].values())
    assert [int(ev.n_entries[g]) for g in (-1, 0, 2)] == [n, int((groups == 0).sum()), int((groups == 2).sum())]
    # aggregated, the same users in two groups that both have members
    two = (groups // 2).astype(groups.dtype)
    agg = run(FullEvaluator(True, 2, torch.from_numpy(two)))
    assert len(agg) == 36
    for prefix, rows in (('', np.ones(n, bool)), ('group_0_', two == 0), ('group_1_', two == 1)):
        for t, k in enumerate(EVAL_KS):
            for j, name in enumerate(NAMES):
                want = per_user[rows, t, j].astype(np.float64).mean()
                assert abs(agg[f'{prefix}{name}@{k}'] - want) <= 1e-12 * abs(want), (what, prefix, name, k)
                got3 = float(ev.group_metrics[{'': -1, 'group_0_': 0, 'group_1_': 2}[prefix]][f'{name}@{k}']) / rows.sum()
                assert abs(got3 - want) <= 1e-12 * abs(want), (what, prefix, name, k)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['quantised', 'hidden'])
def test_mf_eval_loop_two_chunks(kind):
    """16384 + 37 users of integer tables (exact scores, real ties): the loop's two chunks against one call over all users
    bit for bit, against the exact expected ids, and the group sums on the device."""
    import torch
    from hassaku_amd import hip_ops
    from hassaku_amd.algorithms.sgd_alg import SGDMatrixFactorization
    n_users, n_items, D = 16384 + 37, 160, 8
    c = selection_case((n_users, n_users, n_items, D, 100, None), kind, True, 0, n_items)
    users = np.arange(n_users)
    S = c['U'].astype(np.float64) @ c['I'].astype(np.float64).T
    for b in ((None if c['Ub'] is None else c['Ub'].astype(np.float64)[:, None]),
              (None if c['Ib'] is None else c['Ib'].astype(np.float64)[None, :]), c['gb']):
        if b is not None:
            S = S + b
    _, exp_ids = expected_topk(S, c['pairs'], users, 100, 0)
    rng = np.random.RandomState(5)
    n_lab = rng.randint(0, 7, size=n_users)
    n_lab[[5, 16384, 16420]] = [120, 0, 9]
    lab_pairs = np.concatenate([np.stack([np.full(m, q), rng.choice(n_items, size=m, replace=False)], 1)
                                for q, m in enumerate(n_lab) if m])
    lp, li = csr_from_pairs(lab_pairs, n_users)
    ep, ei = csr_from_pairs(c['pairs'], n_users)
    label_rows = [li[lp[q]:lp[q + 1]] for q in users]
    model = SGDMatrixFactorization(n_users, n_items, D, c['Ub'] is not None, c['Ib'] is not None, c['gb'] is not None)
    with torch.no_grad():
        model.user_embeddings.weight.copy_(torch.from_numpy(c['U']))
        model.item_embeddings.weight.copy_(torch.from_numpy(c['I']))
        if c['Ib'] is not None:
            model.item_bias.weight.copy_(torch.from_numpy(c['Ib'])[:, None])
        if c['Ub'] is not None:
            model.user_bias.weight.copy_(torch.from_numpy(c['Ub'])[:, None])
        if c['gb'] is not None:
            model.global_bias.copy_(torch.from_numpy(c['gb']))
    model = model.to('cuda')
    arrays = {'label_indptr': _dev(lp), 'label_indices': _dev(li), 'excl_indptr': _dev(ep), 'excl_indices': _dev(ei)}
    dataset = types.SimpleNamespace(n_users=n_users, n_items=n_items, device_arrays=lambda device: arrays)
    from hassaku_amd.eval.eval import FullEvaluator
    res, chunks = _evaluate(model, dataset, FullEvaluator(False, 0), 'cuda')
    assert chunks == [(0, 16384), (16384, 37)]
    per_user = _stack(res)
    assert per_user.shape == (n_users, 4, 3) and per_user.dtype == np.float32
    # one call over all users
    u_all = torch.arange(n_users, device='cuda')
    _, ids, _ = hip_ops.mf_eval_topk(*model.tables(), u_all, 100, arrays['excl_indptr'], arrays['excl_indices'])
    met = hip_ops.rank_metrics(ids, u_all, arrays['label_indptr'], arrays['label_indices'], EVAL_KS).cpu().numpy()
    assert np.array_equal(per_user.view(np.int32), met.view(np.int32))
    assert np.array_equal(ids.cpu().numpy(), exp_ids)
    _hold_to_restatement(per_user, exp_ids, label_rows, kind)
    groups = np.where(rng.rand(n_users) < .4, 0, 2).astype(np.int64)
    _hold_groups(lambda ev: _evaluate(model, dataset, ev, 'cuda')[0], per_user, groups, kind)
    torch.cuda.synchronize()


def _sparse_case(reverse):
    """A small ItemKNN problem and its restatement: 300 users x 150 items, cosine, k = 20."""
    from hassaku_amd.data.csr import UserItemCsr
    from hassaku_amd.data.synthetic import generate
    d = generate(300, 150, 6000, seed=11)
    flip = (lambda a: 299 - a) if reverse else (lambda a: a)
    train = UserItemCsr.from_pairs(flip(d.train[:, 0]), d.train[:, 1], 300, 150)
    val = UserItemCsr.from_pairs(flip(d.val[:, 0]), d.val[:, 1], 300, 150)
    users = np.arange(300)
    neigh = kr.neighbours(kr.dense_binary(train.indptr, train.indices, 300, 150).T.copy(), 'cosine', 20, 0.)
    pred = kr.predictions('iknn', users, (train.indptr, train.indices), neigh, 300, 150)
    _, ids = kr.masked_topk(pred, [train.row(int(q)) for q in users], 100)
    return train, val, ids


@pytest.mark.gpu
@pytest.mark.parametrize('reverse', [False, True])
def test_sparse_eval_loop_five_chunks(monkeypatch, reverse):
    """ItemKNN through _hip_sparse_eval in five chunks (64, 64, 64, 64, 44 users, one reused score buffer) against the
    single-chunk run bit for bit and against the restatement; in both user orders the last chunk's users rank other items
    than the users whose rows the buffer held before, so a stale row would show.  Then the group sums, and the calibration
    decorator around the evaluator."""
    import torch
    from hassaku_amd.algorithms.knn_algs import ItemKNN
    from hassaku_amd.eval import eval as eval_mod
    from hassaku_amd.eval.eval import FullEvaluator, FullEvaluatorCalibrationDecorator
    train, val, exp_ids = _sparse_case(reverse)
    assert (exp_ids[256:300] != exp_ids[192:236]).any(1).all()
    m = ItemKNN('cosine', 20, 0.)
    m.fit(train)
    ep, ei = train.to_device('cuda')
    lp, li = val.to_device('cuda')
    arrays = {'label_indptr': lp, 'label_indices': li, 'excl_indptr': ep, 'excl_indices': ei}
    dataset = types.SimpleNamespace(n_users=300, n_items=150, device_arrays=lambda device: arrays)
    single, chunks = _evaluate(m, dataset, FullEvaluator(False, 0), m.device)
    assert chunks == [(0, 300)]
    rng = np.random.RandomState(3)
    item_tags = torch.from_numpy(rng.dirichlet(np.ones(6), 150).astype(np.float32))
    user_tags = torch.from_numpy(rng.dirichlet(np.ones(6), 300).astype(np.float32))
    decorated = lambda: FullEvaluatorCalibrationDecorator(FullEvaluator(False, 0), item_tags, user_tags)    # noqa: E731
    single_cal, _ = _evaluate(m, dataset, decorated(), m.device)
    monkeypatch.setattr(eval_mod, 'SPARSE_EVAL_CHUNK_BYTES', 64 * 8 * 150)
    multi, chunks = _evaluate(m, dataset, FullEvaluator(False, 0), m.device)
    assert chunks == [(0, 64), (64, 64), (128, 64), (192, 64), (256, 44)]
    assert sorted(multi) == sorted(single) and len(multi) == 12
    for name in single:
        assert np.array_equal(multi[name].view(np.int32), single[name].view(np.int32)), name
    per_user = _stack(multi)
    _hold_to_restatement(per_user, exp_ids, [val.row(int(q)) for q in range(300)], ('iknn', reverse))
    multi_cal, chunks = _evaluate(m, dataset, decorated(), m.device)
    assert len(chunks) == 5 and sorted(multi_cal) == sorted(single_cal) and len(multi_cal) == 24
    for name in single_cal:
        assert np.array_equal(multi_cal[name], single_cal[name], equal_nan=True), name
        assert np.isfinite(multi_cal[name]).all()
    for name in single:
        assert np.array_equal(multi_cal[name], single[name]), name
    groups = np.where(rng.rand(300) < .5, 0, 2).astype(np.int64)
    _hold_groups(lambda ev: _evaluate(m, dataset, ev, m.device)[0], per_user, groups, ('iknn', reverse))
    torch.cuda.synchronize()
