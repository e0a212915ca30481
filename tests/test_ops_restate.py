"""CPU self-check of tests/ops_restate.py and of the claims the cases of tests/test_unfused_ops.py rest on: the tile rule
against the table of DESIGN section 3, the exactness precondition of every exact case, and the coverage of the dispatch
boundaries.  No GPU, no torch."""
import numpy as np
import pytest

import ops_cases as C
import ops_restate as R

# DESIGN section 3, written out by hand for every dimension the cases use: D -> (V, NCH, FULL)
DESIGN_TILES = {
    1: (1, 1, False), 3: (1, 1, False), 63: (1, 1, False), 65: (1, 2, False), 127: (1, 2, False), 129: (1, 4, False),
    255: (1, 4, False), 257: (1, 8, False), 511: (1, 8, False),
    2: (2, 1, False), 6: (2, 1, False), 30: (2, 1, False), 126: (2, 1, False), 130: (2, 2, False), 254: (2, 2, False),
    258: (2, 4, False), 402: (2, 4, False), 1022: (2, 8, False),
    4: (4, 1, False), 60: (4, 1, False), 64: (4, 1, False), 252: (4, 1, False), 256: (4, 1, True), 260: (4, 2, False),
    508: (4, 2, False), 512: (4, 2, True), 1020: (4, 4, False), 1024: (4, 4, True), 1028: (4, 8, False),
    2044: (4, 8, False), 2048: (4, 8, True),
    513: None, 1026: None, 2052: None,
}


def test_tile_agrees_with_the_design_table():
    used = set(C.D_LADDER) | set(C.K_LADDER_D) | set(C.BIAS_D) | set(C.D_REFUSED) | {C.BATCH_LIMIT['D']}
    assert used <= set(DESIGN_TILES), sorted(used - set(DESIGN_TILES))
    for D, want in DESIGN_TILES.items():
        assert R.tile(D) == want, D
    for D in C.D_REFUSED:           # the refusals sit just past each alignment's limit
        assert R.max_dim(D) < D <= R.max_dim(D) + 4 and R.tile(R.max_dim(D)) is not None
    assert R.score_rows_buffered(64) == 4 and R.score_rows_buffered(1024) == 2


def test_clamp_rule():
    idx = np.array([-1, 0, 4, 5, 1 << 40, -(1 << 40)])
    assert R.clamp(idx, 5).tolist() == [0, 0, 4, 0, 0, 0]
    assert R.is_bad(idx, 5) and not R.is_bad(np.array([0, 4]), 5)


def test_restatement_on_a_hand_computed_case():
    U = np.array([[1., 2.], [3., -1.]])
    I = np.array([[2., 0.], [-1., 4.], [5., 5.]])
    Ib, Ub, gb = np.array([10., 20., 30.]), np.array([100., 200.]), np.array([1000.])
    u, i = np.array([1, 0]), np.array([[2, 0, 2], [1, 1, 0]])
    s, scale, n = R.scores(U, I, Ib, Ub, gb, u, i)
    assert s.tolist() == [[10 + 200 + 30 + 1000, 6 + 200 + 10 + 1000, 10 + 200 + 30 + 1000],
                          [7 + 100 + 20 + 1000, 7 + 100 + 20 + 1000, 2 + 100 + 10 + 1000]]
    assert scale[0, 0] == 20 + 200 + 30 + 1000 and scale[1, 0] == 9 + 100 + 20 + 1000 and n == 5
    s2, _, n2 = R.scores(U, I, None, Ub, None, u, i)
    assert s2[0, 1] == 6 + 200 and n2 == 3
    s0, _, n0 = R.scores(None, None, Ib, Ub, None, u, i)
    assert s0.tolist() == [[230, 210, 230], [120, 120, 110]] and n0 == 2
    g = np.array([[1., -2., 3.], [0.5, 0.5, -1.]])
    G = R.backward(U, I, u, i, g)
    gU, sU, nU = G['user_emb']
    assert gU.tolist() == [[-1 + 0 - 2, 4 + 0 - 0], [4 * 5 - 2 * 2, 4 * 5]] and nU.tolist() == [[3, 3], [3, 3]]
    assert sU[1].tolist() == [4 * 5 + 2 * 2, 4 * 5]
    gI, sI, nI = G['item_emb']
    assert gI.tolist() == [[-2 * 3 - 1, 2 - 2], [1, 2], [12, -4]] and nI[:, 0].tolist() == [2, 2, 2]
    assert sI[0].tolist() == [6 + 1, 2 + 2]
    assert G['item_bias'][0].tolist() == [-3., 1., 4.] and G['item_bias'][1].tolist() == [3., 1., 4.]
    assert G['user_bias'][0].tolist() == [0., 2.] and G['user_bias'][2].tolist() == [3, 3]
    assert G['global_bias'][0].tolist() == [2.] and G['global_bias'][1].tolist() == [8.] and G['global_bias'][2][0] == 6
    G0 = R.backward(None, None, u, i, g, 2, 3)
    assert 'user_emb' not in G0 and G0['item_bias'][0].tolist() == [-3., 1., 4.]


def test_bounds_handle_zero_scale_and_subnormals():
    scale = np.array([0.0, 1.0, 2.0 ** -140])
    ref = np.array([0.0, 0.5, 2.0 ** -141])
    tol = R.grad_bound(scale, np.array([0, 3, 3]), ref)
    assert tol[0] == 0.0 and tol[1] == 4 * 2.0 ** -24 and tol[2] == 4 * 2.0 ** -149
    tol = R.scores_bound(64, scale, ref)
    assert tol[0] == 0.0 and tol[1] == (4 + 6 + 3) * 2.0 ** -24 and tol[2] == 13 * 2.0 ** -149


@pytest.mark.parametrize('case', C.mf_cases() + C.bias_cases(), ids=lambda c: c['name'])
def test_exact_cases_meet_the_exactness_precondition(case):
    T = C.tables(case, 'exact')
    for k, a in T.items():
        if a is not None:
            assert np.array_equal(a, np.round(a)), k
    (s, scale, _), grads, status = C.expected(case, T)
    assert R.is_exact(scale), ('scores', scale.max())
    for name, (g, gscale, n) in grads.items():
        assert R.is_exact(gscale), (name, gscale.max())
        assert (g[gscale == 0] == 0).all() and (gscale[n == 0] == 0).all(), name
    # the spare rows are named by no valid index: their gradients stay zero whatever the case
    for name in ('item_emb', 'item_bias'):
        if name in grads:
            assert not np.any(grads[name][2][list(C.SPARE_ITEMS)]), name
    for name in ('user_emb', 'user_bias'):
        if name in grads:
            assert not np.any(grads[name][2][C.SPARE_USER]), name
    assert status == (1 if case['bad'] else 0)
    if case['bad']:      # the clamped entry reads row 0, so row 0 has terms
        assert grads['user_bias' if case['bad'][0] == 'u' else 'item_bias'][2][0] > 0


def test_batch_limit_case_meets_the_precondition():
    case = C.batch_limit_case()
    T = C.tables(case, 'exact')
    s, scale, _ = R.scores(T['user_emb'], T['item_emb'], T['item_bias'], T['user_bias'], T['global_bias'],
                           case['u'], case['i'])
    assert case['B'] > 65535 and R.is_exact(scale)


def test_cases_reach_every_dispatch_boundary():
    mf = C.mf_cases()
    cov = C.coverage(mf)
    assert {t[:2] for t in cov['tiles']} == C.ALL_TILES
    assert {t[2] for t in cov['tiles']} == {False, True}
    for V, NCH, FULL in cov['tiles']:
        assert not FULL or V == 4
    # the D ladder by itself holds every (V, NCH) pair and both FULL values
    ladder = {R.tile(D) for D in C.D_LADDER}
    assert {t[:2] for t in ladder} == C.ALL_TILES and {t[2] for t in ladder} == {False, True}
    assert {t for t in ladder if t[2]} == {(4, 1, True), (4, 2, True), (4, 4, True), (4, 8, True)}
    # every K residue mod 4 at both R, every remainder of a pass against R, a second workgroup, retired waves
    assert cov['residues'] >= {(Rb, r) for Rb in (2, 4) for r in range(4)}
    assert cov['remainders'] >= {(2, 0), (2, 1)} | {(4, r) for r in range(4)}
    assert cov['second_group'] and cov['retired_waves'] and cov['ragged_y']
    k_cov = C.coverage(C.k_ladder_cases())
    assert k_cov['residues'] >= {(Rb, r) for Rb in (2, 4) for r in range(4)} and k_cov['second_group']
    for D in C.K_LADDER_D:      # a ragged last workgroup along x: some but not all of its waves live
        assert any(0 < C.column_geometry(K, D)['retired_waves'] < 4 and K > 512 for K in C.K_LADDER)
    # bias sets: all eight; bad indices: every value at every column, for both index arrays
    assert {c['bias'] for c in C.bias_set_cases()} == set(C.BIAS_SETS) and len(set(C.BIAS_SETS)) == 8
    bad = {c['bad'][:2] + (c['bad'][3],) for c in C.bad_cases() if c['bad'][0] == 'i'}
    assert bad == {('i', t, col) for t in C.BAD_VALUES for col in C.BAD_COLS}
    assert {c['bad'][1] for c in C.bad_cases() if c['bad'][0] == 'u'} == set(C.BAD_VALUES)
    # dim == 0: B * K on both sides of 256 (one workgroup of the score kernel), global bias present and absent
    bl = C.bias_ladder_cases()
    assert any(c['B'] * c['K'] < 256 for c in bl) and any(c['B'] * c['K'] > 256 for c in bl)
    assert {c['bias'][2] for c in bl} == {True, False}
    assert {c['B'] for c in bl} == set(C.BIAS_LADDER_B)
    names = [c['name'] for c in mf + C.bias_cases()]
    assert len(names) == len(set(names))
