"""Numpy restatement of the device negative sampler's draw-by-draw law ("sampler law"), written from the
statement and not from the kernels: tests/test_sampler_exact.py holds every form of the sampler to it with integer
equality.

Slot (b, n) of a batch drawn with 64-bit `seed` and 64-bit stream id `t`, catalogue size I, the user's sorted positives R:

  key      (seed mod 2^32, seed >> 32)
  counter  (b, n, t mod 2^32, (((t >> 32) << 16) | j) mod 2^32)   for the attempt block j = 0 .. 4095
  words    w0..w3 = Philox4x32-10(counter, key)

  uniform  the words in order: m = w * I (exact, 64 bits); m mod 2^32 < 2^32 mod I: the word is spent (biased zone), no
           candidate; otherwise the candidate is m >> 32.  The first candidate outside R is the draw.
  alias    the pairs (w0, w1), (w2, w3) in order: the column from the pair's first word as above (a biased-zone word spends
           the pair); u = (second word >> 8) * 2^-24 in fp32; the candidate is the column if u < prob[column], else
           alias[column].
  give up  after 4096 blocks: the last candidate formed (0 if none ever was), and a flag.

Only the low 16 bits of t >> 32 reach the counter: stream ids that differ only above bit 48 collide.
"""
import numpy as np

N_BLOCKS = 4096
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11).  ctr: four uint32 arrays (or
    scalars) of one shape, key: two python ints -> four uint32 arrays."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=np.uint64)) & _LO for c in ctr)
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = _M0 * c0             # < 2^64: exact
        p1 = _M1 * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _LO, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _LO
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


class Draws:
    """Per slot [B, n_neg]: neg (int64), candidates formed, biased-zone words (alias: pairs) spent, attempt blocks
    used, gave_up."""

    def __init__(self, shape):
        self.neg = np.zeros(shape, dtype=np.int64)
        self.n_cand = np.zeros(shape, dtype=np.int64)
        self.n_spent = np.zeros(shape, dtype=np.int64)
        self.n_blocks = np.zeros(shape, dtype=np.int64)
        self.gave_up = np.zeros(shape, dtype=bool)

    @property
    def past_block0(self):
        return int((self.n_blocks > 1).sum())


def _array_table(prob, alias):
    prob, alias = np.asarray(prob, dtype=np.float32), np.asarray(alias, dtype=np.int64)
    return lambda cols: (prob[cols], alias[cols])


def draw_negatives(seed, stream, users, n_neg, indptr, indices, n_items, alias=None, b_offset=0, n_blocks=N_BLOCKS):
    """The negatives of batch rows b = 0 .. len(users) - 1 (row b belongs to user users[b]; the counter's first word is
    b + b_offset), n_neg slots each.  indptr / indices: CSR of the sorted positives.  alias: None (uniform), a pair of
    arrays (prob fp32 [I], alias [I]), or a callable cols -> (prob[cols], alias[cols]) for tables too large to keep on
    the host."""
    seed, stream, n_items = int(seed) & (2 ** 64 - 1), int(stream) & (2 ** 64 - 1), int(n_items)
    assert 0 < n_items < 2 ** 31
    users = np.asarray(users, dtype=np.int64)
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    B = len(users)
    out = Draws((B, n_neg))
    key = (seed % 2 ** 32, seed >> 32)
    zone = np.uint64(2 ** 32 % n_items)
    # membership per row: row r of the CSR is ascending, rows follow each other -> r * 2^32 + item is ascending overall,
    # so one searchsorted resolves every open slot against its own row
    lens = np.diff(indptr)
    row_of = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
    keyed = row_of * 2 ** 32 + indices
    assert np.all(np.diff(keyed) > 0), 'rows must be sorted and duplicate-free'

    def member(slot_users, cand):
        q = slot_users * 2 ** 32 + cand
        pos = np.searchsorted(keyed, q)
        return (pos < len(keyed)) & (keyed[np.minimum(pos, len(keyed) - 1)] == q)

    table = None if alias is None else (alias if callable(alias) else _array_table(*alias))
    flat = lambda a: a.reshape(-1)
    neg, n_cand, n_spent, blocks, gave = (flat(a) for a in (out.neg, out.n_cand, out.n_spent, out.n_blocks, out.gave_up))
    sb, sn = (flat(a) for a in np.meshgrid(np.arange(B, dtype=np.int64), np.arange(n_neg, dtype=np.int64), indexing='ij'))
    open_ = np.arange(B * n_neg)           # flat indices of the slots that have not drawn yet
    hi = ((stream >> 32) << 16)
    for j in range(n_blocks):
        if len(open_) == 0:
            break
        w = philox4x32_10((sb[open_] + b_offset, sn[open_], np.full(len(open_), stream % 2 ** 32), np.full(len(open_), (hi | j) % 2 ** 32)),
                          key)
        blocks[open_] = j + 1
        alive = np.ones(len(open_), dtype=bool)          # within this block
        for a in (range(4) if table is None else (0, 2)):
            m = w[a].astype(np.uint64) * np.uint64(n_items)
            spent = (m & _LO) < zone
            n_spent[open_[alive & spent]] += 1
            form = alive & ~spent
            if not form.any():
                continue
            cand = (m[form] >> _S32).astype(np.int64)
            if table is not None:
                u = (w[a + 1][form] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
                p, al = table(cand)
                cand = np.where(u < np.asarray(p, dtype=np.float32), cand, np.asarray(al, dtype=np.int64))
            idx = open_[form]
            n_cand[idx] += 1
            neg[idx] = cand                              # the last candidate formed, until a later one replaces it
            ok = ~member(users[sb[idx]], cand)
            alive[np.flatnonzero(form)[ok]] = False
        open_ = open_[alive]
    gave[open_] = True
    return out


def fused_batch(seed, t, coo_user, coo_item, order, start, batch, n_neg, indptr, indices, n_items, alias=None, b_offset=0):
    """The batch a fused step builds after `t` earlier steps: (u [batch], items [batch, 1 + n_neg], Draws)."""
    pos = np.arange(start, start + batch)
    if order is not None:
        pos = np.asarray(order, dtype=np.int64)[pos]
    u = np.asarray(coo_user, dtype=np.int64)[pos]
    d = draw_negatives(seed, t, u, n_neg, indptr, indices, n_items, alias=alias, b_offset=b_offset)
    items = np.concatenate([np.asarray(coo_item, dtype=np.int64)[pos][:, None], d.neg], axis=1)
    return u, items, d
