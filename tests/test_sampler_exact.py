"""Every form of the device negative sampler against the numpy restatement of its law (tests/sampler_restate.py, DESIGN.md
"sampler law"): which integer slot (b, n) of step t holds is a pure function of (seed, t, b, n, the user's row, I, the
alias table), so every comparison here is np.array_equal on integers -- no tolerance, no statistics.

  A  k_sample_negatives, uniform        B  k_sample_negatives, alias table        C  k_prep_sample (eager fused step)
  D  k_prep_sample from the graph descriptor, k_prep_sample_group                 E  hsk_ride_sample_body (bitmap / staged /
                                                                                     global membership test, partly filled wave)

The CPU tests hold the restatement's Philox to published known answers, the restatement to its own invariants, and
every case to the condition it is there for (biased-zone words met, slots past attempt block 0, the boundary rows in a
checked batch, the rows' LAST entries observable), from the restatement's counts: a GPU case cannot pass vacuously.

Not varied here (read once per process): HSK_PIPE_S_PER_WAVE (default 8 positives per wave: 1 and 64, where the wave's
first positive is also its last or every lane hands one out, stay untested), HSK_GROUP, HSK_FWD_PARTS.  The slots
0 .. 6 of a grouped graph's last group cannot be read through the API; the bit-equality tests of test_hip_parity.py tie
their effect to single steps.  k_shard_sample is held through tests/test_dist.py (every rank's kept entries == the
single-GPU sample) once C holds k_prep_sample.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import csr_from_pairs
import sampler_restate as sr

SEED = 0x9E3779B97F4A7C15
T_A = (3 << 32) | 5
T_B = (7 << 32) | 5          # differs from T_A in the high word only
GAVE_UP = 2                  # HSK_STATUS_SAMPLER_GAVE_UP


# ---------------------------------------------------------------------------------------------------
# Philox and the restatement itself
# ---------------------------------------------------------------------------------------------------
PHILOX_KAT = [   # Random123's kat_vectors for philox4x32-10
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_known_answers():
    from oracle.oracle import _philox4x32_10
    for ctr, key, out in PHILOX_KAT:
        assert tuple(int(x[0]) for x in sr.philox4x32_10(ctr, key)) == out
        assert tuple(int(np.atleast_1d(x)[0]) for x in _philox4x32_10(*[np.array([c], dtype=np.uint32) for c in ctr], *key)) == out
    # vectorised == element by element
    rng = np.random.RandomState(0)
    c = rng.randint(0, 2 ** 32, size=(4, 50), dtype=np.uint64)
    v = sr.philox4x32_10(tuple(c), (123, 0xfedcba98))
    for e in (0, 17, 49):
        assert [int(x[e]) for x in v] == [int(x[0]) for x in sr.philox4x32_10(tuple(int(c[k, e]) for k in range(4)), (123, 0xfedcba98))]


def _scalar_draw(seed, t, b, n, row, I):
    """One uniform slot straight from the statement, in python integers."""
    row, last = set(int(x) for x in row), 0
    for j in range(sr.N_BLOCKS):
        w = sr.philox4x32_10((b, n, t % 2 ** 32, (((t >> 32) << 16) | j) % 2 ** 32), (seed % 2 ** 32, seed >> 32))
        for x in w:
            m = int(x[0]) * I
            if m % 2 ** 32 < 2 ** 32 % I:
                continue
            last = m >> 32
            if last not in row:
                return last
    return last


def test_restatement_equals_a_scalar_reading_of_the_statement():
    rng = np.random.RandomState(1)
    for I in (3, 97, 3 << 29):
        ptr, idx, users = _rows_for(I, rng)
        d = sr.draw_negatives(SEED, T_A, users, 5, ptr, idx, I)
        for b in range(len(users)):
            for n in range(5):
                assert d.neg[b, n] == _scalar_draw(SEED, T_A, b, n, idx[ptr[users[b]]:ptr[users[b] + 1]], I), (I, b, n)


def _assert_invariants(d, users, ptr, idx, I):
    assert d.neg.min() >= 0 and d.neg.max() < I
    ok = ~d.gave_up
    for b in range(d.neg.shape[0]):
        row = idx[ptr[users[b]]:ptr[users[b] + 1]]
        assert not np.isin(d.neg[b][ok[b]], row).any(), b
    assert np.all(d.n_cand[ok] >= 1) and np.all(d.n_blocks[ok] >= 1)


# ---------------------------------------------------------------------------------------------------
# A / B: the stand-alone sampler's cases
# ---------------------------------------------------------------------------------------------------
A_SIZES = [2, 3, 97, 65536, 3 << 29, (1 << 31) - 2]
A_NEG = 200          # lanes stride past 64


def _rows_for(I, rng, n_users=10, n_rows=24):
    """A few short rows (user 0: none, 1: {0}, 2: {I - 1}) and u_idx with repeats in no order: b is the batch position."""
    rows = [np.zeros(0, np.int64), np.array([0]), np.array([I - 1])]
    for _ in range(n_users - 3):
        k = rng.randint(0, min(I - 1, 40) + 1)
        rows.append(np.unique(rng.randint(0, I, size=k))[:max(0, min(k, I - 1))])
    pairs = np.array([(u, it) for u, r in enumerate(rows) for it in r], dtype=np.int64)
    ptr, idx = csr_from_pairs(pairs, n_users)
    users = rng.randint(0, n_users, size=n_rows).astype(np.int64)
    users[:3] = (2, 0, 1)
    return ptr, idx, users


@functools.lru_cache(maxsize=None)
def _case_a(I):
    ptr, idx, users = _rows_for(I, np.random.RandomState(I % 1000003))
    return ptr, idx, users, {t: sr.draw_negatives(SEED, t, users, A_NEG, ptr, idx, I) for t in (T_A, T_B)}


@functools.lru_cache(maxsize=None)
def _case_self_targeted():
    """I = 3 * 2^29: a third of the integers drawn against near-empty rows go into the users' rows, then draw again."""
    I = 3 << 29
    ptr, idx, users, ref = _case_a(I)
    first = ref[T_A]
    hit = np.zeros(first.neg.shape, dtype=bool)
    hit.reshape(-1)[::3] = True
    old = [(u, it) for u in range(len(ptr) - 1) for it in idx[ptr[u]:ptr[u + 1]]]
    new = [(users[b], first.neg[b, n]) for b, n in zip(*np.nonzero(hit))]
    ptr2, idx2 = csr_from_pairs(np.array(old + new, dtype=np.int64), len(ptr) - 1)
    return I, ptr2, idx2, users, first, hit, sr.draw_negatives(SEED, T_A, users, A_NEG, ptr2, idx2, I)


# (15 of 16 leaves ONE item: every slot must find it whatever the words are -- that case holds the walk over the blocks to
# its end, not the integers; 13 of 16 is its observable neighbour)
DENSE = [(97, 92), (16, 15), (16, 13)]


@functools.lru_cache(maxsize=None)
def _case_dense(I, held):
    rng = np.random.RandomState(held)
    ptr, idx = csr_from_pairs(np.stack([np.zeros(held, np.int64), rng.permutation(I)[:held]], axis=1), 1)
    users = np.zeros(2, dtype=np.int64)
    return ptr, idx, users, sr.draw_negatives(SEED, T_A, users, A_NEG, ptr, idx, I)


@functools.lru_cache(maxsize=None)
def _case_give_up():
    I = 16
    ptr, idx = np.array([0, I], dtype=np.int64), np.arange(I, dtype=np.int32)
    users = np.zeros(2, dtype=np.int64)
    return I, ptr, idx, users, sr.draw_negatives(SEED, T_A, users, 3, ptr, idx, I)


@functools.lru_cache(maxsize=None)
def _case_alias_small():
    I, U = 60, 12
    rng = np.random.RandomState(2)
    ptr, idx = csr_from_pairs(np.argwhere(rng.rand(U, I) < 0.3), U)
    p = rng.rand(I) ** 6              # strong skew
    p[rng.permutation(I)[:15]] = 0.0  # exact zeros
    from hassaku_amd.hip_ops import build_alias_table
    prob, alias = build_alias_table(p / p.sum())
    users = rng.randint(0, U, size=24).astype(np.int64)
    return I, ptr, idx, users, prob, alias, p, sr.draw_negatives(SEED, T_A, users, A_NEG, ptr, idx, I, alias=(prob, alias))


ALIAS_BIG_I, ALIAS_BIG_ROWS = 3 << 24, 256      # 2^32 mod I = 2^24: one first word in 256 is in the biased zone


def _alias_big_rows():
    return _rows_for(ALIAS_BIG_I, np.random.RandomState(11), n_rows=ALIAS_BIG_ROWS)


def test_cpu_stand_alone_cases_exercise_what_they_claim():
    for I in A_SIZES:
        ptr, idx, users, ref = _case_a(I)
        assert len(idx) > 0 and len(np.unique(users)) < len(users) and not np.all(np.diff(users) >= 0)
        for t in (T_A, T_B):
            _assert_invariants(ref[t], users, ptr, idx, I)
            assert not ref[t].gave_up.any()
        assert not np.array_equal(ref[T_A].neg, ref[T_B].neg)      # the stream id's high word reaches the counter
        if I == 3 << 29:
            assert int(ref[T_A].n_spent.reshape(-1)[:256].sum()) >= 50      # a quarter of all words is in the biased zone
        if I == 65536:
            assert ref[T_A].n_spent.sum() == 0                              # a power of two has no biased zone
    # ... up to bit 48 only: the documented limit
    ptr, idx, users, ref = _case_a(97)
    assert np.array_equal(sr.draw_negatives(SEED, T_A + (1 << 48), users, A_NEG, ptr, idx, 97).neg, ref[T_A].neg)
    assert not np.array_equal(sr.draw_negatives(SEED, T_A + (1 << 47), users, A_NEG, ptr, idx, 97).neg, ref[T_A].neg)

    I, ptr2, idx2, users, first, hit, second = _case_self_targeted()
    _assert_invariants(second, users, ptr2, idx2, I)
    assert hit.sum() >= 1000 and np.all(second.neg[hit] != first.neg[hit]) and np.all(second.n_cand[hit] >= 2)
    untouched = second.n_cand == first.n_cand                               # (a slot may also meet another slot's integer)
    assert np.array_equal(second.neg[untouched], first.neg[untouched]) and untouched[~hit].mean() > 0.99

    for I, held in DENSE:
        ptr, idx, users, d = _case_dense(I, held)
        _assert_invariants(d, users, ptr, idx, I)
        assert d.neg.size == 400 and d.past_block0 > 100 and not d.gave_up.any(), (I, d.past_block0)

    I, ptr, idx, users, d = _case_give_up()
    assert d.gave_up.all() and np.all(d.n_cand + d.n_spent == 4 * sr.N_BLOCKS) and np.all(d.n_blocks == sr.N_BLOCKS)

    I, ptr, idx, users, prob, alias, p, d = _case_alias_small()
    _assert_invariants(d, users, ptr, idx, I)
    assert (p == 0).sum() >= 10 and not np.isin(d.neg, np.flatnonzero(p == 0)).any()   # a zero-probability item is never drawn
    assert d.past_block0 > 100 and not d.gave_up.any()      # (two candidates per block, rows of ~ 18 of 60 items)

    # the big alias case's table lives on the device; which pairs are spent before the first candidate is formed does
    # not depend on it, and with rows this short the first candidate is (all but) always the draw
    ptr, idx, users = _alias_big_rows()
    keep = np.ones(ALIAS_BIG_I // (1 << 20), dtype=np.float32)   # stand-in: every column keeps itself
    d = sr.draw_negatives(SEED, T_A, users, A_NEG, ptr, idx, ALIAS_BIG_I,
                          alias=lambda cols: (keep[cols >> 20], cols))
    assert int(d.n_spent.sum()) >= 100 and not d.gave_up.any()


# ---------------------------------------------------------------------------------------------------
# C / D / E: batches of the fused step
# ---------------------------------------------------------------------------------------------------
class Fused:
    """A data set for the fused step, its order, and the restated batches."""

    def __init__(self, n_users, n_items, dim, pairs, order, alias=None, seed=SEED):
        self.U, self.I, self.D, self.pairs, self.order, self.alias, self.seed = n_users, n_items, dim, pairs, order, alias, seed
        self.ptr, self.idx = csr_from_pairs(pairs, n_users)
        assert len(self.idx) == len(pairs), 'duplicate pairs'

    @functools.lru_cache(maxsize=None)
    def batch(self, t, start, B, N, use_order=True):
        return sr.fused_batch(self.seed, t, self.pairs[:, 0], self.pairs[:, 1], self.order if use_order else None, start, B, N,
                              self.ptr, self.idx, self.I, alias=self.alias)

    def state(self, B, N, **kw):
        from hassaku_amd import hip_ops as ops
        g = torch.Generator().manual_seed(5)
        dev = lambda a, dt=None: (torch.from_numpy(np.ascontiguousarray(a)).to(dt) if dt else torch.from_numpy(np.ascontiguousarray(a))).cuda()
        self.t = [(torch.randn(self.U, self.D, generator=g) * 0.05).cuda(), (torch.randn(self.I, self.D, generator=g) * 0.05).cuda(),
                  torch.zeros(self.I).cuda()]
        alias = None if self.alias is None else (dev(self.alias[0]), dev(self.alias[1]))
        st = ops.BprMfFusedState(*self.t, lr=1e-3, wd=1e-4, max_batch=B, max_cols=N + 1, seed=self.seed, csr_indptr=dev(self.ptr),
                                 csr_indices=dev(self.idx), coo_user=dev(self.pairs[:, 0], torch.int32),
                                 coo_item=dev(self.pairs[:, 1], torch.int32), alias=alias, **kw)
        self.order_dev = dev(self.order)
        st.st.nnz = len(self.order)        # the runs walk `order`, which may name an interaction more than once
        return st

    def assert_last_batch(self, st, t, start, B, N, use_order=True, what=''):
        u, i = (x.cpu().numpy() for x in st.last_batch(B, N + 1))
        ru, ri, _ = self.batch(t, start, B, N, use_order)
        assert np.array_equal(u, ru), (what, t, 'users')
        assert np.array_equal(i[:, 0], ri[:, 0]), (what, t, 'positives')
        bad = np.argwhere(i != ri)
        assert len(bad) == 0, (what, t, len(bad), 'slots differ; first (b, column, got, restated):',
                               [(int(b), int(c), int(i[b, c]), int(ri[b, c])) for b, c in bad[:5]])


def _random_pairs(rng, n_users, n_items, dens):
    pairs = np.argwhere(rng.rand(n_users, n_items) < dens)
    return pairs[rng.permutation(len(pairs))]


C_SHAPE = dict(U=120, I=300, D=64, B=96, N=20)
C_BATCHES = [(0, 96), (96, 96), (192, 40), (232, 96)]     # (start, batch) of t = 0 .. 3: a ragged batch in between


@functools.lru_cache(maxsize=None)
def _case_c(kind):
    rng = np.random.RandomState(3)
    U, I, D = C_SHAPE['U'], C_SHAPE['I'], C_SHAPE['D']
    alias = None
    if kind == 'rows':     # I = 3000, users 0 / 1 hold exactly 1024 / 1025 positives: the LDS row limit of k_prep_sample
        I = 3000
        mask = rng.rand(U, I) < 0.005
        for u, n in ((0, 1024), (1, 1025)):
            mask[u] = False
            mask[u, rng.permutation(I)[:n]] = True
        pairs = np.argwhere(mask)
        pairs = pairs[rng.permutation(len(pairs))]
    else:
        pairs = _random_pairs(rng, U, I, 0.05)
    order = rng.permutation(len(pairs))
    if kind == 'rows':     # both of them in every batch, as neighbours
        for start, nb in C_BATCHES:
            for k, u in enumerate((0, 1, 0)):
                order[start + 7 + k] = rng.choice(np.flatnonzero(pairs[:, 0] == u))
    if kind == 'alias':
        from hassaku_amd.hip_ops import build_alias_table
        alias = build_alias_table(np.bincount(pairs[:, 1], minlength=I).astype(np.float64) ** 0.75 + 1e-3)
    return Fused(U, I, D, pairs, order, alias)


D_PLAIN = dict(U=900, I=700, D=128, B=2048, N=10, steps=64)      # one replayed graph, k_prep_sample from the descriptor
D_GROUP = dict(U=300, I=400, D=402, B=128, N=50, steps=128)      # two replayed graphs, k_prep_sample_group


@functools.lru_cache(maxsize=None)
def _case_d(grouped):
    sh = D_GROUP if grouped else D_PLAIN
    rng = np.random.RandomState(4)
    pairs = _random_pairs(rng, sh['U'], sh['I'], 0.15)
    need = (sh['steps'] + 1) * sh['B']
    order = np.concatenate([rng.permutation(len(pairs)) for _ in range(-(-need // len(pairs)))])
    return Fused(sh['U'], sh['I'], sh['D'], pairs, order)


# E: D = 256, N = 17, B = 2048: the item-partitioned forward with P = 2, whose launches carry the riding sampler
E_D, E_N, E_PER_WAVE = 256, 17, 8
E_LENS = (1, 256, 257, 1024, 1025)          # users 0 .. 4 hold exactly this many positives
E_RUNS = (3, 4, 5)                          # steps_sampled runs on one state; the last batches: t = 2, 6, 11
E_CHECKED = (2, 6, 11)
E_CASES = {     # name: (n_items, alias, batch)
    'bitmap-6000': (6000, False, 2048), 'bitmap-32768': (32768, False, 2048), 'staged-32769': (32769, False, 2048),
    'staged-40000': (40000, False, 2048), 'bitmap-6000-alias': (6000, True, 2048), 'bitmap-6000-b2050': (6000, False, 2050),
    'staged-32769-b2050': (32769, False, 2050),
}
# users whose positives sit in the batch positions that one wave of the riding sampler handles as its k = 0 .. 7: a long
# row (bitmap set and cleared over > 1024 entries, or searched in global memory) in front of a one-entry row, and so on
E_WAVE_USERS = ((0, 0, (4, 0, 3, 1, 2, 0, 4, 2)), (5, 2, (0, 4, 1, 3, 0, 2, 3, 4)))     # (workgroup, wave, users by k)


def _ride_positions(B, bid, wave):
    """Batch positions of the riding sampler's wave (bid, wave), k = 0 .. per_wave - 1 (hsk_sampler.h: positive k of a
    wave is b = (k * n_blocks + bid) * 4 + wave with n_blocks = ceil(B / (4 * per_wave)))."""
    n_blocks = -(-B // (4 * E_PER_WAVE))
    return [(k * n_blocks + bid) * 4 + wave for k in range(E_PER_WAVE)]


@functools.lru_cache(maxsize=None)
def _case_e(name):
    I, popular, B = E_CASES[name]
    rng = np.random.RandomState(I % 1000 + B)
    U, half = 300, I // 2
    # rows of users 0 .. 4: all but the last entry in the lower half of the catalogue; the last entry starts as a
    # placeholder at the top and is then moved onto an integer the sampler DRAWS for that user in a checked batch, so
    # that entry 255 / 256 / 1023 / 1024 of a row -- the last one a register, a staging loop or a search range reaches --
    # decides a draw
    rows = [np.sort(rng.permutation(half)[:n - 1]) for n in E_LENS]
    pairs = [(u, it) for u, r in enumerate(rows) for it in r] + [(u, I - 1 - u) for u in range(len(E_LENS))]
    rest = np.argwhere(rng.rand(U - len(E_LENS), I) < 40.0 / I)
    rest[:, 0] += len(E_LENS)
    pairs = np.concatenate([np.array(pairs, dtype=np.int64), rest])
    n_special = int((pairs[:, 0] < len(E_LENS)).sum())
    order = rng.randint(n_special, len(pairs), size=sum(E_RUNS) * B)
    by_user = [np.flatnonzero(pairs[:, 0] == u) for u in range(len(E_LENS))]
    for t in range(sum(E_RUNS)):
        order[t * B + rng.permutation(B)[:200]] = rng.randint(0, n_special, size=200)      # ~ 1 / 80 / 80 of them by row length
        for bid, wave, us in E_WAVE_USERS:
            for b, u in zip(_ride_positions(B, bid, wave), us):
                if b < B:
                    order[t * B + b] = rng.choice(by_user[u])
    alias = None
    if popular:
        from hassaku_amd.hip_ops import build_alias_table
        alias = build_alias_table(rng.rand(I) ** 3 + 1e-3)
    # move the placeholders
    t0 = E_CHECKED[0]
    probe = Fused(U, I, E_D, pairs, order, alias)
    bu, bi, _ = probe.batch(t0, t0 * B, B, E_N)
    taken = set()
    for u in range(len(E_LENS)):
        drawn = bi[bu == u, 1:].reshape(-1)
        drawn = [int(x) for x in drawn if x >= half and x < I - len(E_LENS) and int(x) not in taken]
        assert drawn, ('no draw in the upper half for user', u)
        taken.add(drawn[0])
        pairs[np.flatnonzero((pairs[:, 0] == u) & (pairs[:, 1] == I - 1 - u))[0], 1] = drawn[0]
    return Fused(U, I, E_D, pairs, order, alias), B


def test_cpu_fused_cases_exercise_what_they_claim():
    for kind in ('order', 'alias', 'rows'):
        c = _case_c(kind)
        for t, (start, nb) in enumerate(C_BATCHES):
            for use_order in ((True, False) if kind == 'order' else (True,)):
                u, i, d = c.batch(t, start, nb, C_SHAPE['N'], use_order)
                _assert_invariants(d, u, c.ptr, c.idx, c.I)
                assert not d.gave_up.any()
                if kind == 'rows':
                    assert {0, 1} <= set(u.tolist()) and d.n_cand[u == 1].max() >= 2 and d.n_cand[u == 0].max() >= 2
        if kind == 'rows':
            assert list(np.diff(c.ptr)[:2]) == [1024, 1025]
    # successive steps draw different negatives for the same slot
    c = _case_c('order')
    assert not np.array_equal(c.batch(0, 0, 96, 20)[2].neg, c.batch(1, 0, 96, 20)[2].neg)


@pytest.mark.parametrize('name', list(E_CASES))
def test_cpu_riding_cases_exercise_what_they_claim(name):
    c, B = _case_e(name)
    assert tuple(np.diff(c.ptr)[:len(E_LENS)]) == E_LENS
    assert (B % (4 * E_PER_WAVE) != 0) == (B == 2050)          # 2050: the last wave of the hand-out is partly filled
    for t in E_CHECKED:
        u, i, d = c.batch(t, t * B, B, E_N)
        _assert_invariants(d, u, c.ptr, c.idx, c.I)
        assert not d.gave_up.any() and set(range(len(E_LENS))) <= set(u.tolist())
        for bid, wave, us in E_WAVE_USERS:
            pos = [b for b in _ride_positions(B, bid, wave) if b < B]
            assert list(u[pos]) == list(us[:len(pos)])
    # every boundary row's LAST entry, and everything beyond entry 256 of the long rows, decides a draw of a checked batch
    t = E_CHECKED[0]
    u, i, d = c.batch(t, t * B, B, E_N)
    for usr, n in enumerate(E_LENS):
        if n == 1:
            continue
        lo = c.ptr[usr]
        for cut in ([n - 1] if n <= 256 else [n - 1, 256]):      # the row without its last entry / cut to 256 entries
            keep = np.ones(len(c.idx), dtype=bool)
            keep[lo + cut:lo + n] = False
            ptr2 = c.ptr.copy()
            ptr2[usr + 1:] -= n - cut
            d2 = sr.draw_negatives(c.seed, t, u, E_N, ptr2, c.idx[keep], c.I, alias=c.alias)
            assert not np.array_equal(d2.neg[u == usr], d.neg[u == usr]), (usr, cut)
            assert np.array_equal(d2.neg[u != usr], d.neg[u != usr])


# ---------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------
def _dev(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dt) if dt else t).cuda()


def _gpu_draw(ptr, idx, I, users, n_neg, t, alias=None, expect_status=0):
    from hassaku_amd import hip_ops as ops
    status = ops.new_status('cuda')
    neg = ops.sample_negatives_uniform(_dev(ptr), _dev(idx, torch.int32), I, _dev(users), n_neg, seed=SEED, stream_id=t,
                                       status=status, alias=alias).cpu().numpy()
    assert int(status.item()) == expect_status
    return neg


def _assert_same(got, d, what):
    bad = np.argwhere(got != d.neg)
    assert len(bad) == 0, (what, len(bad), 'slots differ; first (b, n, got, restated, candidates, spent):',
                           [(int(b), int(n), int(got[b, n]), int(d.neg[b, n]), int(d.n_cand[b, n]), int(d.n_spent[b, n]))
                            for b, n in bad[:5]])


@pytest.mark.gpu
@pytest.mark.parametrize('I', A_SIZES)
def test_stand_alone_uniform_draws(I):
    ptr, idx, users, ref = _case_a(I)
    got = {t: _gpu_draw(ptr, idx, I, users, A_NEG, t) for t in (T_A, T_B)}
    for t in (T_A, T_B):
        _assert_same(got[t], ref[t], (I, hex(t)))
    assert not np.array_equal(got[T_A], got[T_B])
    # the documented limit: bits 48 and up of the stream id do not reach the counter, bit 47 does
    assert np.array_equal(_gpu_draw(ptr, idx, I, users, A_NEG, T_A + (1 << 48)), got[T_A])
    _assert_same(_gpu_draw(ptr, idx, I, users, A_NEG, T_A + (1 << 47)),
                 sr.draw_negatives(SEED, T_A + (1 << 47), users, A_NEG, ptr, idx, I), (I, 'bit 47'))


@pytest.mark.gpu
def test_stand_alone_self_targeted_rows_move_to_the_next_candidate():
    I, ptr2, idx2, users, first, hit, second = _case_self_targeted()
    got = _gpu_draw(ptr2, idx2, I, users, A_NEG, T_A)
    _assert_same(got, second, 'self-targeted')
    assert np.all(got[hit] != first.neg[hit])


@pytest.mark.gpu
@pytest.mark.parametrize('I,held', DENSE)
def test_stand_alone_dense_rows(I, held):
    ptr, idx, users, d = _case_dense(I, held)
    _assert_same(_gpu_draw(ptr, idx, I, users, A_NEG, T_A), d, ('dense', I))


@pytest.mark.gpu
def test_stand_alone_give_up_returns_the_last_candidate():
    I, ptr, idx, users, d = _case_give_up()
    _assert_same(_gpu_draw(ptr, idx, I, users, 3, T_A, expect_status=GAVE_UP), d, 'give-up')


@pytest.mark.gpu
def test_stand_alone_alias_draws_small_table():
    I, ptr, idx, users, prob, alias, p, d = _case_alias_small()
    _assert_same(_gpu_draw(ptr, idx, I, users, A_NEG, T_A, alias=(_dev(prob), _dev(alias))), d, 'alias 60')


@pytest.mark.gpu
def test_stand_alone_alias_draws_large_table_with_biased_zone():
    """I = 3 * 2^24 with any table at all (prob uniform in [0, 1), alias uniform in [0, I), both made on the device): the
    restatement gathers the columns it meets from the device."""
    I = ALIAS_BIG_I
    ptr, idx, users = _alias_big_rows()
    g = torch.Generator(device='cuda').manual_seed(3)
    prob = torch.rand(I, device='cuda', generator=g)
    alias = torch.randint(0, I, (I,), device='cuda', generator=g, dtype=torch.int32)

    def table(cols):
        c = torch.from_numpy(cols).cuda()
        return prob[c].cpu().numpy(), alias[c].cpu().numpy()
    d = sr.draw_negatives(SEED, T_A, users, A_NEG, ptr, idx, I, alias=table)
    assert int(d.n_spent.sum()) >= 100 and not d.gave_up.any()
    _assert_same(_gpu_draw(ptr, idx, I, users, A_NEG, T_A, alias=(prob, alias)), d, 'alias 3 * 2^24')


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['order', 'no-order', 'alias', 'rows'])
def test_eager_fused_step_batches(kind):
    c = _case_c('order' if kind == 'no-order' else kind)
    B, N = C_SHAPE['B'], C_SHAPE['N']
    st = c.state(B, N)
    for t, (start, nb) in enumerate(C_BATCHES):
        st.step_sampled(None if kind == 'no-order' else c.order_dev, start, nb, N)
        c.assert_last_batch(st, t, start, nb, N, use_order=kind != 'no-order', what=kind)
    st.check_status()


@pytest.mark.gpu
@pytest.mark.parametrize('grouped', [False, True])
def test_replayed_graph_batches(grouped):
    sh = D_GROUP if grouped else D_PLAIN
    c = _case_d(grouped)
    B, N, n = sh['B'], sh['N'], sh['steps']
    st = c.state(B, N)
    st.steps_sampled(c.order_dev, 0, n, B, N)
    assert st.graph_replays() == n // 64 and st.step_count == n
    c.assert_last_batch(st, n - 1, (n - 1) * B, B, N, what='replayed')           # grouped: slot 7 of the last group
    st.step_sampled(c.order_dev, n * B, B, N)                                   # an eager step behind the run
    c.assert_last_batch(st, n, n * B, B, N, what='eager after replay')
    st.check_status()


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(E_CASES))
def test_riding_sampler_batches(name):
    """B = 2050: hsk_ride_sample_body hands positive k of wave (bid, w) position (k * 65 + bid) * 4 + w and stops a wave at
    its first position >= B (ascending in k), and k_fwd_part / the item and user passes bound every row by b < B -- the
    shape is supported; the waves from (workgroup 57, wave 2) on then hold 7 positives instead of 8."""
    c, B = _case_e(name)
    st = c.state(B, E_N)
    assert st.batch_columns(B, E_N + 1) == E_N + 2
    t = 0
    for run in E_RUNS:
        st.steps_sampled(c.order_dev, t * B, run, B, E_N)
        t += run
        # (a run's first two batches are prepared by launches of their own: the last batch of a run of >= 3 rode)
        c.assert_last_batch(st, t - 1, (t - 1) * B, B, E_N, what=name)
    assert st.pipelined_steps() == sum(E_RUNS)
    st.check_status()
