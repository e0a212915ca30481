"""Plain restatements for the lazy-replay tests (numpy, float64; nothing here touches the library).

zero_grad_chain      torch's single-tensor AdamW / Adam-with-L2 / Adagrad-with-L2 arithmetic for a ZERO gradient, step by
                     step -- what a row outside every batch goes through, whoever replays it and however late.
zero_grad_chain_bound  the same chain together with a running bound on what fp32 arithmetic may lose against it.
adam_scalars         the per-step fp32 scalars (step_size, sqrt(bc2), 1/sqrt(bc2)) by hsk_make_adamw_consts' formula.
schedule             hand-built batches: which rows a step touches, hence how far behind a row is when it is touched.

The rounding bound.  u = 2^-24 is one rounding of an fp32 result, relative to that result (half an ulp at most; a
hardware v_sqrt_f32 / v_rcp_f32 is held to 1 ulp = 2 u).  Every fp32 operation of one optimiser step is listed below
with its count of roundings, each scaled by the magnitude of the quantity it rounds -- "of the element's own scale" --
and errors already carried by the operands are propagated to first order (|d(xy)| <= |x| dy + |y| dx, d sqrt(v) =
dv / (2 sqrt(v)), d(1/x) = dx / x^2).  Constants that the library rounds from double once (decay, 1 - beta1, beta2,
1 - beta2, lr / bc1, 1 / sqrt(bc2), eps, wd) count as one rounding of the product they enter.  The default build's
update term is  -step_size * m * rcp(fma(sqrt(v), rbc2_sqrt, eps)):  sqrt 2 u, rcp 2 u, i.e. the "3 ulp on the update
term" of csrc/hsk_common.h together with the fma's own rounding; the IEEE build's sqrtf and two divisions round once
each and stay inside the same count.
"""
import numpy as np

U24 = 2.0 ** -24
OPTS = ('adamw', 'adam', 'adagrad')
TAB_LEN = 65536            # HSK_ADAM_TAB_LEN (csrc/hsk_fused.hip)
REQUIRED_BACKLOGS = (0, 1, 2, 62, 63, 64, 65, 66, 126, 127, 128, 129, 191, 192, 193)


def default_eps(opt, eps=None):
    if eps is not None:
        return eps
    return 1e-10 if opt == 'adagrad' else 1e-8


def zero_grad_chain_bound(opt, p, m, v, t_from, t_to, lr, wd, b1=0.9, b2=0.999, eps=None):
    """Steps t_from + 1 .. t_to (1-based step numbers, as torch counts them) with g = 0 on float64 copies of p, m, v.
    -> (p, m, v, Ep, Em, Ev): the float64 results and, per element, a bound on |fp32 result - float64 result| for an
    fp32 evaluation that starts from the same (fp32-representable) p, m, v and rounds as the module docstring lists."""
    assert opt in OPTS
    eps = default_eps(opt, eps)
    p, m, v = (np.array(a, dtype=np.float64) for a in (p, m, v))
    Ep, Em, Ev = np.zeros_like(p), np.zeros_like(m), np.zeros_like(v)
    u = U24
    for t in range(int(t_from) + 1, int(t_to) + 1):
        if opt == 'adamw':
            # p.mul_(1 - lr * wd): the constant's rounding + the product's
            p = p * (1.0 - lr * wd)
            Ep = Ep * (1.0 - lr * wd) + 2 * u * np.abs(p)
            g, Eg = 0.0, 0.0
        else:
            # grad = grad.add(p, alpha=wd): wd's rounding + the product's
            g = wd * p
            Eg = wd * Ep + 2 * u * np.abs(g)
        if opt == 'adagrad':
            # state_sum.addcmul_(g, g); std = sqrt(state_sum) + eps; p.addcdiv_(g, std, value=-lr)
            v = v + g * g
            Ev = Ev + 2 * np.abs(g) * Eg + u * np.abs(v)
            s = np.sqrt(v)
            Es = np.where(s > 0, Ev / (2 * np.where(s > 0, s, 1.0)), np.sqrt(Ev)) + 2 * u * s
            den = s + eps
            Eden = Es + u * den + u * eps
            num = lr * g
            Enum = lr * Eg + 2 * u * np.abs(num)
        else:
            # exp_avg.lerp_(g, 1 - b1): (g - m) rounds, w1 is rounded, the fma rounds
            d = g - m
            m_new = m + (1.0 - b1) * d
            Em = (1.0 - (1.0 - b1)) * Em + (1.0 - b1) * Eg + 2 * u * (1.0 - b1) * np.abs(d) + u * np.abs(m_new)
            m = m_new
            # exp_avg_sq.mul_(b2).addcmul_(g, g, value=1 - b2): b2 and v * b2 round; (1 - b2), (1 - b2) g round; the fma rounds
            v_new = b2 * v + (1.0 - b2) * g * g
            Ev = b2 * Ev + 2 * (1.0 - b2) * np.abs(g) * Eg + 2 * u * b2 * np.abs(v) + 2 * u * (1.0 - b2) * g * g + u * np.abs(v_new)
            v = v_new
            bc1 = 1.0 - b1 ** t
            bc2s = np.sqrt(1.0 - b2 ** t)
            s = np.sqrt(v)
            Es = np.where(s > 0, Ev / (2 * np.where(s > 0, s, 1.0)), np.sqrt(Ev)) + 2 * u * s
            # denom = sqrt(v) / bc2_sqrt + eps: the rounded 1 / bc2_sqrt, the fma (or the division and the sum), eps
            den = s / bc2s + eps
            Eden = Es / bc2s + u * s / bc2s + u * den + u * eps
            num = (lr / bc1) * m
            Enum = (lr / bc1) * Em + 2 * u * np.abs(num)       # step_size's rounding + the product's
        r = 1.0 / den
        Er = Eden * r * r + 2 * u * r                           # rcp: 1 ulp
        upd = num * r
        Eupd = Enum * r + np.abs(num) * Er
        p = p - upd
        Ep = Ep + Eupd + u * np.abs(p)                          # the closing fma (or product and difference)
    return p, m, v, Ep, Em, Ev


def zero_grad_chain(opt, p, m, v, t_from, t_to, lr, wd, b1=0.9, b2=0.999, eps=None):
    """(p, m, v) in float64 after the zero-gradient steps t_from + 1 .. t_to."""
    return zero_grad_chain_bound(opt, p, m, v, t_from, t_to, lr, wd, b1, b2, eps)[:3]


def adam_scalars(lr, t, b1=0.9, b2=0.999):
    """fp32 (step_size, bc2_sqrt, rbc2_sqrt) of steps t (array), by hsk_make_adamw_consts' formula."""
    t = np.asarray(t, dtype=np.float64)
    bc1 = 1.0 - np.power(b1, t)
    bc2 = 1.0 - np.power(b2, t)
    return (np.float32(lr / bc1), np.float32(np.sqrt(bc2)), np.float32(1.0 / np.sqrt(bc2)))


def touches(first, backlogs):
    """Touch steps of a row first touched at step `first` and then again after each of `backlogs` missed steps."""
    out = [int(first)]
    for b in backlogs:
        out.append(out[-1] + int(b) + 1)
    return out


def schedule(n_rows, n_steps, per_step, probes, busy, seed, replace=False, placed=None):
    """Which rows each of the steps 1 .. n_steps touches.

    probes   {row: [steps at which the row is in the batch]} -- and at no other step
    busy     rows that fill the rest of every batch (drawn without replacement unless `replace`)
    placed   {(row, step): [positions]}: the row sits at exactly these positions of that step's batch (several positions
             = a duplicated entry); a probe step without an entry here takes one free position at random
    Rows that are neither probes nor busy are in no batch.

    -> dict(batches = [int64 [per_step]] per step,
            backlogs = {row: [(step, backlog)]} for every touched row, backlog = (step - 1) - last touch (0 before the
                       first), counted from the batches themselves,
            final = int64 [n_rows]: steps missed when the run ends (n_steps - last touch),
            untouched = rows that no batch holds)"""
    rng = np.random.RandomState(seed)
    placed = placed or {}
    busy = np.asarray(busy, dtype=np.int64)
    assert not set(busy.tolist()) & set(probes), 'a probe row must not be in the busy pool'
    for (row, step) in placed:
        assert step in probes[row], (row, step)
    due = {}
    for row, steps in probes.items():
        assert len(set(steps)) == len(steps) and min(steps) >= 1 and max(steps) <= n_steps, (row, steps)
        for s in steps:
            due.setdefault(s, []).append(row)
    batches = []
    for s in range(1, n_steps + 1):
        batch = rng.choice(busy, size=per_step, replace=replace).astype(np.int64)
        free = np.ones(per_step, dtype=bool)
        rows = sorted(due.get(s, []))
        for row in rows:
            for pos in placed.get((row, s), []):
                assert free[pos], (row, s, pos)
                batch[pos], free[pos] = row, False
        for row in rows:
            if (row, s) not in placed:
                pos = rng.choice(np.flatnonzero(free))
                batch[pos], free[pos] = row, False
        batches.append(batch)
    last = np.zeros(n_rows, dtype=np.int64)
    seen = np.zeros(n_rows, dtype=bool)
    backlogs = {}
    for s, batch in enumerate(batches, start=1):
        for row in np.unique(batch).tolist():
            backlogs.setdefault(row, []).append((s, s - 1 - int(last[row])))
            last[row] = s
            seen[row] = True
    return dict(batches=batches, backlogs=backlogs, final=n_steps - last, untouched=np.flatnonzero(~seen))


def backlog_set(sched, rows=None):
    """All backlogs that occur at a touch (of `rows`, or of every row) or at the end of the run."""
    rows = list(sched['backlogs']) if rows is None else rows
    out = set()
    for r in rows:
        out.update(b for _, b in sched['backlogs'].get(r, []))
        out.add(int(sched['final'][r]))
    out.update(int(x) for x in sched['final'][sched['untouched']])
    return out


# ---------------------------------------------------------------------------------------------------
# the probe plans of tests/test_replay_backlog.py (steps are relative to the run's start)
# ---------------------------------------------------------------------------------------------------
LONG_STEPS = 260
# every backlog of REQUIRED_BACKLOGS at a touch, two beyond 250; at the end of the run the probes are 0 .. 126 behind and
# the rows outside every batch LONG_STEPS
LONG_PLAN = [
    touches(1, [0, 1, 2, 62, 63]),        # 1, 2, 4, 7, 70, 134
    touches(3, [64, 65, 66]),             # 3, 68, 134, 201
    touches(2, [126, 127]),               # 2, 129, 257
    touches(1, [128, 129]),               # 1, 130, 260
    touches(1, [191, 65]),                # 1, 193, 259
    touches(2, [192, 62]),                # 2, 195, 258
    touches(3, [193]),                    # 3, 197
    touches(251, [0]),                    # 251, 252
    touches(5, [253]),                    # 5, 259
    touches(1, [63, 64, 65, 63]),         # 1, 65, 130, 196, 260
]

# the same list in 200 steps, for the cases whose steps are expensive (B = 2048): every backlog of REQUIRED_BACKLOGS at a
# touch, the longest 198; a backlog >= 250 does not fit the step count and is not reached there
SHORT_STEPS = 200
SHORT_PLAN = [
    touches(1, [0, 1, 2, 62, 63]),        # 1, 2, 4, 7, 70, 134
    touches(3, [64, 65]),                 # 3, 68, 134
    touches(1, [66, 126]),                # 1, 68, 195
    touches(2, [127, 65]),                # 2, 130, 196
    touches(1, [128, 62]),                # 1, 130, 193
    touches(1, [129, 66]),                # 1, 131, 198
    touches(1, [191]),                    # 1, 193
    touches(2, [192]),                    # 2, 195
    touches(3, [193]),                    # 3, 197
    touches(199, [0]),                    # 199, 200
]

EDGE_STEPS = 200
EDGE_AT = 100         # with start_step = TAB_LEN - EDGE_AT the step TAB_LEN is the run's step EDGE_AT
# a touch at step s after a touch at step l replays the steps l + 1 .. s - 1, handed out in blocks of 64 from l + 1
EDGE_PLAN = [
    [1, 65, 130, 196],     # 63: 2..64 below the table end; 64: 66..129, one block across it; 65: 131..195 above, two blocks
    [40, 106, 173],        # 39 below; 65: 41..104 across + 105 above; 66: 107..172 above
    [10, 138],             # 127: 11..74 below, 75..137 across
    [9, 138],              # 128: 10..73, 74..137 across
    [5, 135],              # 129: 6..69, 70..133 across, 134
    [3, 134],              # 130: 4..67, 68..131 across, 132..133
    [37, 100, 164],        # 62: 38..99 ends just below, touched AT the table end; 63: 101..163 starts just above
    [36, 101, 102, 105],   # 64: 37..100 ends at the table end; 0; 2
    [99, 100, 101, 103],   # eager steps on both sides of the table end; 1
    [198],                 # 197: four blocks, the second across
]
EDGE_BACKLOGS = (0, 1, 2, 62, 63, 64, 65, 66, 127, 128, 129, 130, 197)


def crosses_edge(sched, rows):
    """How the replays of `rows` lie to the table end (the run's step EDGE_AT): counts of replayed 64-step blocks wholly
    below it, containing it, wholly above it -- touches and the closing sweep alike."""
    below = across = above = 0
    spans = []
    for r in rows:
        for s, b in sched['backlogs'].get(r, []):
            spans.append((s - b, s - 1))
        n = len(sched['batches'])
        spans.append((n - int(sched['final'][r]) + 1, n))
    for lo, hi in spans:
        for t0 in range(lo, hi + 1, 64):
            t1 = min(t0 + 63, hi)
            if t1 < EDGE_AT:
                below += 1
            elif t0 > EDGE_AT:
                above += 1
            else:
                across += 1
    return below, across, above
