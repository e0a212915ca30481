"""conf['optimizer'] = adam | adagrad (train/trainer.py:48-51 of the reference): the fused step
with torch.optim.Adam / torch.optim.Adagrad semantics (weight_decay as L2).  Golden vectors G8 come from the
reference's model + torch.optim (oracle/gen_golden.py::gen_g8)."""
import numpy as np
import pytest
import torch

from conftest import PARAM_KEYS, assert_adam_param_close, load_golden, max_norm_err

G8_CASES = ['adam_d32_item', 'adam_d64_all', 'adagrad_d32_item', 'adagrad_d402_all']


def _init(fx):
    return {name: fx['init.' + sk] for sk, name in PARAM_KEYS.items() if 'init.' + sk in fx}


# ---------------------------------------------------------------------------------------------------
# CPU: the oracle against the reference
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', G8_CASES)
def test_oracle_optimizer_on_reference_grads(oracle, case):
    """The optimiser arithmetic alone, fed the reference's own dense gradients of step 1."""
    fx = load_golden(f'g8_opt_{case}.npz')
    opt = str(fx['optimizer'])
    for sk in PARAM_KEYS:
        if 'init.' + sk not in fx:
            continue
        p = fx['init.' + sk].copy()
        m, v = np.zeros_like(p), np.zeros_like(p)
        oracle.opt_step(opt, p, fx['s1.grad.' + sk], m, v, float(fx['lr']), float(fx['wd']), 1)
        assert max_norm_err(p, fx['s1.param.' + sk]) < 1e-6, sk
        assert max_norm_err(v, fx['s1.v.' + sk]) < 1e-6, sk
        if opt == 'adam':
            assert max_norm_err(m, fx['s1.m.' + sk]) < 1e-6, sk


# Adagrad's first steps are lr * g'/(|g'| + 1e-10) with g' = g + wd*p: where the two terms cancel to within ~1e-10 the
# step depends on the last bit of the gradient sum at a rate of up to lr/eps per unit of g' (summation-order noise,
# as for Adam in conftest.assert_adam_param_close, but with eps = 1e-10 and no bias-corrected history yet).  Measured
# oracle-vs-reference on G8: 0.04 % of the elements beyond 1e-5, worst 5.3e-4.  Adam with L2 has no such elements.
def _max_tol(opt):
    return 5e-3 if opt == 'adagrad' else None


def _check_against_golden(P, M, V, fx, step, opt):
    for sk, name in PARAM_KEYS.items():
        # global_bias starts at 0 and has a zero gradient by definition: the reference moves it by +-lr on 1e-9 noise
        if name == 'global_bias' or name not in P:
            continue
        ref = fx[f's{step}.param.{sk}']
        if name == 'user_bias':
            # zero gradient by definition here; the reference adds ~1e-9 autograd noise to g = wd * p ~ 1e-4, i.e.
            # 1e-5 relative on g and 2e-5 on v: hold the parameter, not the moments, and at 1e-4
            assert max_norm_err(P[name], ref.reshape(P[name].shape)) < 1e-4, (step, name)
            continue
        assert_adam_param_close(P[name], ref, (step, name), _max_tol(opt))
        assert_adam_param_close(V[name], fx[f's{step}.v.{sk}'], (step, 'v', name), _max_tol(opt))
        if opt == 'adam':
            assert_adam_param_close(M[name], fx[f's{step}.m.{sk}'], (step, 'm', name))


@pytest.mark.parametrize('case', G8_CASES)
def test_oracle_three_steps_match_reference(oracle, case):
    fx = load_golden(f'g8_opt_{case}.npz')
    opt = str(fx['optimizer'])
    P = _init(fx)
    tr = oracle.MfOracleTrainer(P['user_emb'], P['item_emb'], P.get('item_bias'), P.get('user_bias'),
                                P.get('global_bias'), lr=float(fx['lr']), wd=float(fx['wd']), optimizer=opt)
    for step in (1, 2, 3):
        loss, _, _, _ = tr.step(fx[f's{step}.u_idx'], fx[f's{step}.i_idx'])
        assert abs(loss - float(fx[f's{step}.loss'])) <= 1e-5 * abs(float(fx[f's{step}.loss']))
        if step in (1, 3):
            _check_against_golden(tr.P, tr.M, tr.V, fx, step, opt)


def test_l2_decay_moves_untouched_rows(oracle):
    """weight_decay is L2 for adam / adagrad: a row outside every batch still sees g = wd * p."""
    fx = load_golden('g8_opt_adagrad_d32_item.npz')
    touched = set()
    for s in (1, 2, 3):
        touched |= set(fx[f's{s}.u_idx'].tolist())
    rows = sorted(set(range(int(fx['n_users']))) - touched)
    assert rows
    p0, p3 = fx['init.user_embeddings.weight'][rows[0]], fx['s3.param.user_embeddings.weight'][rows[0]]
    assert np.abs(p3 - p0).max() > 1e-3        # adagrad's first steps are ~lr per element whatever |g| is


# ---------------------------------------------------------------------------------------------------
# GPU: the HIP path against the reference and the oracle
# ---------------------------------------------------------------------------------------------------
def _dev(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dt) if dt else t).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize('case', G8_CASES)
def test_opt_dense_on_reference_grads(case):
    from hassaku_amd import hip_ops as ops
    fx = load_golden(f'g8_opt_{case}.npz')
    opt = str(fx['optimizer'])
    for sk in PARAM_KEYS:
        if 'init.' + sk not in fx:
            continue
        p = _dev(fx['init.' + sk].copy())
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        ops.opt_dense(opt, p, _dev(fx['s1.grad.' + sk]), m, v, float(fx['lr']), float(fx['wd']), 1)
        assert max_norm_err(p.cpu().numpy(), fx['s1.param.' + sk]) < 1e-6, sk
        assert max_norm_err(v.cpu().numpy(), fx['s1.v.' + sk]) < 1e-6, sk
        if opt == 'adam':
            assert max_norm_err(m.cpu().numpy(), fx['s1.m.' + sk]) < 1e-6, sk
        else:
            assert not m.any()                   # adagrad leaves exp_avg alone


DENSE_GRID = 2048 * 256 * 4      # elements one pass of hsk_opt_dense's capped grid covers (float4 per thread)


@pytest.fixture(scope='module', params=[1, 2, 3, 4, 5, 7, DENSE_GRID, DENSE_GRID + 1, DENSE_GRID + 3, DENSE_GRID + 4,
                                        DENSE_GRID + 5])
def dense_inputs(request):
    """n, p, non-zero moments and a gradient over 1e-12 .. 1e3 with both signs and exact zeros: built once per size and
    shared by the three optimisers' cases (pytest runs a module-scoped parameter's cases together)."""
    n = request.param
    rng = np.random.RandomState(n % 9973)
    p = (rng.randn(n) * 0.05).astype(np.float32)
    m = (rng.randn(n) * 1e-3).astype(np.float32)
    v = ((0.25 + rng.rand(n)) * 1e-6).astype(np.float32)
    g = (np.sign(rng.randn(n)) * 10.0 ** rng.uniform(-12, 3, size=n)).astype(np.float32)
    g[rng.rand(n) < 0.1] = 0.0
    g[:min(n, 4)] = np.array([1e3, -1e-12, 0.0, -1e3], np.float32)[:min(n, 4)]
    g[-1] = np.float32(-7.0)                           # a gradient the scalar tail cannot miss
    return n, p, m, v, g


@pytest.mark.gpu
@pytest.mark.parametrize('opt', ['adamw', 'adam', 'adagrad'])
def test_opt_dense_every_tail_and_late_steps(oracle, opt, dense_inputs):
    """hsk_opt_dense, the optimiser of every autograd-path model, against oracle.opt_step: sizes around the float4 body /
    scalar tail and one pass of the capped grid (above it the grid-stride loop runs a second round), steps up to far
    beyond the bias corrections' saturation, preloaded moments, wd = 0 and 1e-2; g = None is a zero gradient, bit for bit."""
    from hassaku_amd import hip_ops as ops
    n, p0, m0, v0, g = dense_inputs
    gd = _dev(g)
    for step in (1, 2, 1000, 65536, 10 ** 6):
        for wd in (0.0, 1e-2):
            p, m, v = _dev(p0.copy()), _dev(m0.copy()), _dev(v0.copy())
            ops.opt_dense(opt, p, gd, m, v, 1e-3, wd, step)
            rp, rm, rv = p0.copy(), m0.copy(), v0.copy()
            oracle.opt_step(opt, rp, g, rm, rv, 1e-3, wd, step)
            what = (opt, n, step, wd)
            assert max_norm_err(v.cpu().numpy(), rv) < 1e-6, what
            if opt == 'adagrad':
                assert np.array_equal(m.cpu().numpy(), m0), what
            else:
                assert max_norm_err(m.cpu().numpy(), rm) < 1e-6, what
            assert_adam_param_close(p.cpu().numpy(), rp, what, _max_tol(opt))
            assert not np.array_equal(p.cpu().numpy()[-1:], p0[-1:]), what      # the last element was updated
    for wd in (0.0, 1e-2):
        a = [_dev(x.copy()) for x in (p0, m0, v0)]
        b = [_dev(x.copy()) for x in (p0, m0, v0)]
        ops.opt_dense(opt, a[0], None, a[1], a[2], 1e-3, wd, 1000)
        ops.opt_dense(opt, b[0], torch.zeros_like(gd), b[1], b[2], 1e-3, wd, 1000)
        for x, y in zip(a, b):
            assert torch.equal(x, y), (opt, n, wd)


@pytest.mark.gpu
@pytest.mark.parametrize('case', G8_CASES)
def test_fused_step_three_steps_vs_golden(case):
    from hassaku_amd import hip_ops as ops
    fx = load_golden(f'g8_opt_{case}.npz')
    opt = str(fx['optimizer'])
    P = _init(fx)
    t = {k: _dev(v.reshape(-1) if k not in ('user_emb', 'item_emb') else v) for k, v in P.items()}
    B, K = fx['s1.i_idx'].shape
    st = ops.BprMfFusedState(t['user_emb'], t['item_emb'], t.get('item_bias'), t.get('user_bias'), t.get('global_bias'),
                             lr=float(fx['lr']), wd=float(fx['wd']), max_batch=B, max_cols=K, optimizer=opt)
    for step in (1, 2, 3):
        st.step(_dev(fx[f's{step}.u_idx']), _dev(fx[f's{step}.i_idx']))
        st.flush()
        assert abs(st.last_loss() - float(fx[f's{step}.loss'])) <= 1e-5 * abs(float(fx[f's{step}.loss']))
        if step in (1, 3):
            got = {k: v.cpu().numpy() for k, v in t.items()}
            M = {k: v.cpu().numpy() for k, v in st.m.items() if v is not None}
            V = {k: v.cpu().numpy() for k, v in st.v.items() if v is not None}
            _check_against_golden(got, M, V, fx, step, opt)
    st.check_status()


@pytest.mark.gpu
@pytest.mark.parametrize('opt', ['adam', 'adagrad'])
def test_lazy_user_update_is_bitwise_the_dense_sweep(opt):
    """L2 decay makes the 'zero-gradient' step of an untouched row depend on the row itself (g = wd * p): the replay
    still reproduces the dense sweep bit for bit, across the flush boundary."""
    import test_hip_parity as T
    from hassaku_amd import hip_ops as ops
    dense, l0 = T._run_random_steps(ops, 150, lazy=False, optimizer=opt)
    lazy, l1 = T._run_random_steps(ops, 150, lazy=True, optimizer=opt)
    assert l0 == l1
    for k in dense:
        assert np.array_equal(dense[k], lazy[k]), k
    base, _ = T._run_random_steps(ops, 150, lazy=True)           # and it is not AdamW under another name
    assert not np.array_equal(base['user_emb'], lazy['user_emb'])


@pytest.mark.gpu
@pytest.mark.parametrize('opt', ['adam', 'adagrad'])
def test_fused_steps_match_oracle_on_random_batches(oracle, opt):
    from hassaku_amd import hip_ops as ops
    rng = np.random.RandomState(8)
    U, I, D, B, N = 90, 70, 48, 40, 12
    P = {'user_emb': (rng.randn(U, D) * 0.05).astype(np.float32), 'item_emb': (rng.randn(I, D) * 0.05).astype(np.float32),
         'item_bias': (rng.randn(I) * 0.1).astype(np.float32), 'user_bias': (rng.randn(U) * 0.1).astype(np.float32)}
    lr = 1e-3 if opt == 'adam' else 1e-2
    t = {k: _dev(v.copy()) for k, v in P.items()}
    st = ops.BprMfFusedState(t['user_emb'], t['item_emb'], t['item_bias'], t['user_bias'], lr=lr, wd=1e-3, max_batch=B,
                             max_cols=N + 1, optimizer=opt)
    tr = oracle.MfOracleTrainer(P['user_emb'], P['item_emb'], P['item_bias'], P['user_bias'], lr=lr, wd=1e-3, optimizer=opt)
    for _ in range(5):
        u = rng.randint(0, U, size=B).astype(np.int64)
        i = rng.randint(0, I, size=(B, N + 1)).astype(np.int64)
        st.step(_dev(u), _dev(i))
        loss_ref, _, _, _ = tr.step(u, i)
        assert abs(st.last_loss() - loss_ref) <= 1e-5 * abs(loss_ref)
    st.flush()
    for k in P:
        assert_adam_param_close(t[k].cpu().numpy(), tr.P[k], k, _max_tol(opt))
    st.check_status()
