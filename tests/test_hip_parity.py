"""GPU parity: the HIP path (through the C ABI) against the CPU oracle and the reference's golden vectors."""
import os
import numpy as np
import pytest
import torch

from conftest import G1_CASES, PARAM_KEYS, assert_adam_param_close, csr_from_pairs, load_golden, max_norm_err

pytestmark = pytest.mark.gpu

RTOL = 1e-5          # north_star tolerance: 1e-5 relative fp32


def dev(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def _init(fx):
    return {name: fx['init.' + sk] for sk, name in PARAM_KEYS.items() if 'init.' + sk in fx}


def _flat(a):
    return None if a is None else a.reshape(-1)


@pytest.fixture(scope='module')
def ops():
    from hassaku_amd import hip_ops
    return hip_ops


def test_library_reports_gfx950(ops):
    import ctypes
    from hassaku_amd import _lib
    lib = _lib.load()
    cu, wave = ctypes.c_int32(), ctypes.c_int32()
    arch = ctypes.create_string_buffer(64)
    _lib.check(lib.hsk_device_info(ctypes.byref(cu), ctypes.byref(wave), arch, 64))
    assert wave.value == 64
    assert arch.value.decode().startswith('gfx950'), arch.value


@pytest.mark.parametrize('case', G1_CASES)
def test_scores_loss_backward_vs_golden(ops, oracle, case):
    fx = load_golden(f'g1_step_{case}.npz')
    P = _init(fx)
    u, i = dev(fx['s1.u_idx']), dev(fx['s1.i_idx'])
    U, I = dev(P['user_emb']), dev(P['item_emb'])
    Ib, Ub, gb = dev(_flat(P.get('item_bias'))), dev(_flat(P.get('user_bias'))), dev(_flat(P.get('global_bias')))
    status = ops.new_status(U.device)
    logits = ops.mf_scores(U, I, Ib, Ub, gb, u, i, status)
    np.testing.assert_allclose(logits.cpu().numpy(), fx['s1.logits'], rtol=RTOL, atol=1e-9)
    loss, g = ops.bpr_loss_grad(dev(fx['s1.logits']))
    assert abs(loss.item() - float(fx['s1.loss'])) <= 1e-6 * float(fx['s1.loss'])
    np.testing.assert_allclose(g.cpu().numpy(), fx['s1.grad_logits'], rtol=RTOL, atol=1e-12)
    gU, gI, gIb, gUb, ggb = ops.mf_backward(U, I, u, i, dev(fx['s1.grad_logits']), True, True, True, status)
    assert max_norm_err(gU.cpu().numpy(), fx['s1.grad.user_embeddings.weight']) < RTOL
    assert max_norm_err(gI.cpu().numpy(), fx['s1.grad.item_embeddings.weight']) < RTOL
    if 'item_bias' in P:
        assert max_norm_err(gIb.cpu().numpy(), fx['s1.grad.item_bias.weight'].reshape(-1)) < RTOL
    ops.raise_on_status(status)


def test_default_build_vs_ieee_build_on_golden_steps(ops, monkeypatch):
    """The default build evaluates Adam's sqrt and divisions with v_sqrt_f32 / v_rcp_f32 (1 ulp each); a second build
    (-DHSK_ADAM_IEEE=1, libhassaku_hip_ieee.so) uses the correctly rounded forms, i.e. torch's arithmetic.  Both run
    the reference's three G1 steps: the IEEE build must meet the same bounds as the default one, and the two builds
    are compared with each other.  Measured: they differ by at most 1.9e-5 (max-normalised) on the worst element --
    the same near-cancellation elements where Adam divides by ~eps -- and by more than 1e-5 on ~1e-4 of the elements
    (one element of a 24 x 402 table): the approximations account for < 10 % of the 2e-4 worst-element slack (conftest.ADAM_MAX_TOL), the rest is
    the summation-order effect documented there."""
    from hassaku_amd import _lib
    ieee_path = os.path.join(os.path.dirname(_lib.LIB_PATH), 'libhassaku_hip_ieee.so')
    if not os.path.isfile(ieee_path):
        pytest.skip('libhassaku_hip_ieee.so not built')
    default_lib, ieee_lib = _lib.load(), _lib.open_library(ieee_path)
    worst = 0.0
    for case in ('d64_item', 'd402_item', 'd512_n100', 'd64_dups'):
        fx = load_golden(f'g1_step_{case}.npz')
        B, K = fx['s1.i_idx'].shape
        out = {}
        for tag, lib in (('default', default_lib), ('ieee', ieee_lib)):
            monkeypatch.setattr(_lib, '_lib', lib)
            st, t = _fused_state(ops, _init(fx), float(fx['lr']), float(fx['wd']), B, K)
            for step in (1, 2, 3):
                st.step(dev(fx[f's{step}.u_idx']), dev(fx[f's{step}.i_idx']))
            st.flush()
            st.check_status()
            out[tag] = {k: v.cpu().numpy().copy() for k, v in t.items()}
            del st
        monkeypatch.setattr(_lib, '_lib', default_lib)
        for sk, name in PARAM_KEYS.items():
            if name in ('user_bias', 'global_bias') or name not in out['ieee']:
                continue
            ref = fx[f's3.param.{sk}'].reshape(out['ieee'][name].shape)
            assert_adam_param_close(out['ieee'][name], ref, f'ieee {case} {name}')
            assert_adam_param_close(out['default'][name], ref, f'default {case} {name}')
            worst = max(worst, max_norm_err(out['default'][name], out['ieee'][name]))
            a, b = out['default'][name].astype(np.float64), out['ieee'][name].astype(np.float64)
            assert (np.abs(a - b) / np.abs(b).max() > 1e-5).mean() < 5e-4, (case, name)
    assert worst < 5e-5, worst


@pytest.mark.parametrize('case', G1_CASES)
def test_adamw_dense_on_reference_grads(ops, case):
    fx = load_golden(f'g1_step_{case}.npz')
    for sk in PARAM_KEYS:
        if 'init.' + sk not in fx:
            continue
        p = dev(fx['init.' + sk])
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        ops.adamw_dense(p, dev(fx['s1.grad.' + sk]), m, v, float(fx['lr']), float(fx['wd']), 1)
        assert max_norm_err(p.cpu().numpy(), fx['s1.param.' + sk]) < 1e-6, sk
        assert max_norm_err(m.cpu().numpy(), fx['s1.m.' + sk]) < 1e-6, sk
        assert max_norm_err(v.cpu().numpy(), fx['s1.v.' + sk]) < 1e-6, sk


def _fused_state(ops, P, lr, wd, max_batch, max_cols, **kw):
    t = {k: dev(_flat(v)) if k != 'user_emb' and k != 'item_emb' else dev(v) for k, v in P.items()}
    st = ops.BprMfFusedState(t['user_emb'], t['item_emb'], t.get('item_bias'), t.get('user_bias'), t.get('global_bias'),
                             lr=lr, wd=wd, max_batch=max_batch, max_cols=max_cols, **kw)
    return st, t


@pytest.mark.parametrize('case', G1_CASES)
def test_fused_step_three_steps_vs_golden(ops, case):
    """hsk_bprmf_train_step on the reference's own batches: loss, parameters, exp_avg, exp_avg_sq."""
    fx = load_golden(f'g1_step_{case}.npz')
    P = _init(fx)
    B, K = fx['s1.i_idx'].shape
    st, t = _fused_state(ops, P, float(fx['lr']), float(fx['wd']), B, K)
    for step in (1, 2, 3):
        st.step(dev(fx[f's{step}.u_idx']), dev(fx[f's{step}.i_idx']))
        st.flush()   # lazy user rows -> current (bit-identical to the dense sweep)
        loss = st.last_loss()
        assert abs(loss - float(fx[f's{step}.loss'])) <= 1e-6 * float(fx[f's{step}.loss']), step
        if step in (1, 3):
            for sk, name in PARAM_KEYS.items():
                if name in ('user_bias', 'global_bias') or name not in P:
                    continue
                ref = fx[f's{step}.param.{sk}'].reshape(-1)
                assert_adam_param_close(t[name].cpu().numpy().reshape(-1), ref, (step, name))
                m_got, v_got = st.m[name].cpu().numpy().reshape(-1), st.v[name].cpu().numpy().reshape(-1)
                m_ref, v_ref = fx[f's{step}.m.{sk}'].reshape(-1), fx[f's{step}.v.{sk}'].reshape(-1)
                if step == 1:   # linear / quadratic in the step-1 gradient: no Adam amplification yet
                    assert max_norm_err(m_got, m_ref) < RTOL and max_norm_err(v_got, v_ref) < RTOL, name
                else:           # later gradients are taken at parameters that already carry it
                    assert_adam_param_close(m_got, m_ref, (step, 'm', name))
                    assert_adam_param_close(v_got, v_ref, (step, 'v', name))
    st.check_status()
    assert st.step_count == 3


def test_fused_step_zero_grad_biases_only_decay(ops):
    """user_bias / global_bias have exactly-zero BPR gradients: AdamW leaves only the weight decay."""
    fx = load_golden('g1_step_d64_all.npz')
    P = _init(fx)
    B, K = fx['s1.i_idx'].shape
    lr, wd = float(fx['lr']), float(fx['wd'])
    st, t = _fused_state(ops, P, lr, wd, B, K)
    for step in (1, 2, 3):
        st.step(dev(fx[f's{step}.u_idx']), dev(fx[f's{step}.i_idx']))
    st.flush()
    d = np.float32(1.0 - lr * wd)
    exp_ub = P['user_bias'].reshape(-1) * d * d * d
    np.testing.assert_allclose(t['user_bias'].cpu().numpy(), exp_ub, rtol=1e-6)
    assert float(st.m['user_bias'].abs().max()) == 0.0 and float(st.v['global_bias'].abs().max()) == 0.0


def test_fused_replay_of_reference_fit(ops, oracle):
    """G4: the exact batch stream of a 2-epoch reference Trainer.fit (ragged last batches included)."""
    fx = load_golden('g4_fit.npz')
    P = {'user_emb': fx['init.user_embeddings.weight'], 'item_emb': fx['init.item_embeddings.weight'],
         'item_bias': fx['init.item_bias.weight']}
    K = int(fx['n_neg']) + 1
    st, t = _fused_state(ops, P, float(fx['lr']), float(fx['wd']), int(fx['batch_size']), K)
    tr = oracle.MfOracleTrainer(P['user_emb'], P['item_emb'], P['item_bias'], lr=float(fx['lr']), wd=float(fx['wd']))
    spe = int(fx['steps_per_epoch'])
    for s in range(int(fx['n_steps'])):
        u, i = fx[f'b{s}.u'], fx[f'b{s}.i']
        st.step(dev(u), dev(i))
        loss_ref, _, _, _ = tr.step(u, i)
        if s % 7 == 0:
            assert abs(st.last_loss() - loss_ref) <= 1e-6 * loss_ref
        if s == spe - 1:
            ep_loss = st.pop_loss_sum() / spe
            assert 0.6 < ep_loss < 0.7
    st.flush()
    assert_adam_param_close(t['user_emb'].cpu().numpy(), fx['final.user_embeddings.weight'], '')
    assert_adam_param_close(t['item_emb'].cpu().numpy(), fx['final.item_embeddings.weight'], '')
    assert_adam_param_close(t['item_bias'].cpu().numpy(), fx['final.item_bias.weight'].reshape(-1), '')
    assert_adam_param_close(t['user_emb'].cpu().numpy(), tr.P['user_emb'], '')
    st.check_status()


@pytest.mark.parametrize('D,U,I,B,N', [(512, 300, 500, 256, 100), (402, 200, 333, 128, 50), (64, 100, 150, 128, 1),
                                        (1024, 64, 200, 32, 200), (33, 50, 101, 17, 3), (6, 20, 100, 5, 130),
                                        # B > 1024: the one-wave-per-positive forward (smaller batches with >= 9
                                        # columns take the workgroup-per-positive kernel)
                                        (402, 300, 333, 1100, 50), (1024, 64, 200, 1040, 20), (33, 50, 101, 1030, 12),
                                        (2048, 40, 90, 24, 30)])
def test_fused_step_vs_oracle_random_shapes(ops, oracle, D, U, I, B, N):
    """BASELINE config shapes (D=512/N=100, D=402/N=50, D=64/N=1, D=1024/N=200), odd sizes, the largest supported
    row (D=2048), both forward kernels; 2 steps."""
    rng = np.random.RandomState(D + B)
    P = {'user_emb': (rng.randn(U, D) * 0.1).astype(np.float32), 'item_emb': (rng.randn(I, D) * 0.1).astype(np.float32),
         'item_bias': (rng.randn(I) * 0.1).astype(np.float32)}
    lr, wd = 3e-4, 4e-5
    st, t = _fused_state(ops, P, lr, wd, B, N + 1)
    tr = oracle.MfOracleTrainer(P['user_emb'], P['item_emb'], P['item_bias'], lr=lr, wd=wd)
    for step in range(2):
        u = rng.randint(0, U, size=B).astype(np.int64)
        i = rng.randint(0, I, size=(B, N + 1)).astype(np.int64)
        st.step(dev(u), dev(i))
        loss_ref, _, _, _ = tr.step(u, i)
        assert abs(st.last_loss() - loss_ref) <= 1e-6 * loss_ref
    st.flush()
    for name in P:
        assert_adam_param_close(st.m[name].cpu().numpy(), tr.M[name], ('m', name))
        assert_adam_param_close(st.v[name].cpu().numpy(), tr.V[name], ('v', name))
        assert_adam_param_close(t[name].cpu().numpy(), tr.P[name], name)
    st.check_status()


@pytest.mark.parametrize('loss', ['sampled_softmax', 'bce', 'bpr'])
def test_large_batch_on_a_mid_size_item_table_vs_oracle(ops, oracle, loss):
    """B = 2048 on an 8 MB item table: the shape the item-partitioned forward is for.  It carries the bpr and bce epilogues;
    sampled softmax must take the un-partitioned kernel (it ran the bpr epilogue there until tests/stress_step.py found it:
    loss 35.3 against 9.26)."""
    D, U, I, B, N = 256, 400, 8000, 2048, 17
    rng = np.random.RandomState(12)
    P = {'user_emb': (rng.randn(U, D) * 0.1).astype(np.float32), 'item_emb': (rng.randn(I, D) * 0.1).astype(np.float32),
         'item_bias': (rng.randn(I) * 0.1).astype(np.float32)}
    lr, wd = 1e-3, 4e-5
    adj = float(np.log(I / N)) if loss == 'sampled_softmax' else 0.0
    st, t = _fused_state(ops, P, lr, wd, B, N + 1, loss=loss, log_adjust=adj)
    assert st.batch_columns(B, N + 1) == (N + 1 if loss == 'sampled_softmax' else N + 2)
    tr = oracle.MfOracleTrainer(P['user_emb'], P['item_emb'], P['item_bias'], lr=lr, wd=wd, loss=loss, log_adjust=adj)
    for step in range(2):
        u = rng.randint(0, U, size=B).astype(np.int64)
        i = rng.randint(0, I, size=(B, N + 1)).astype(np.int64)
        st.step(dev(u), dev(i))
        loss_ref = tr.step(u, i)[0]
        assert abs(st.last_loss() - loss_ref) <= 1e-6 * abs(loss_ref), (step, st.last_loss(), loss_ref)
    st.flush()
    for name in P:
        assert_adam_param_close(t[name].cpu().numpy(), tr.P[name], name)
    st.check_status()


def test_bad_index_is_flagged_not_fatal(ops):
    U = torch.randn(10, 16, device='cuda')
    I = torch.randn(12, 16, device='cuda')
    status = ops.new_status(U.device)
    u = torch.tensor([0, 3], device='cuda')
    i = torch.tensor([[1, 2], [5, 99]], device='cuda')
    ops.mf_scores(U, I, None, None, None, u, i, status)
    with pytest.raises(IndexError):
        ops.raise_on_status(status)


def test_cpu_tensors_are_refused(ops):
    with pytest.raises(RuntimeError):
        ops.mf_scores(torch.randn(4, 8), torch.randn(4, 8), None, None, None, torch.zeros(1, dtype=torch.int64),
                      torch.zeros((1, 2), dtype=torch.int64))


def _run_random_steps(ops, n_steps, lazy, seed=5, U=300, I=200, D=64, B=48, N=9, bias=True, **kw):
    rng = np.random.RandomState(seed)
    P = {'user_emb': (rng.randn(U, D) * 0.05).astype(np.float32), 'item_emb': (rng.randn(I, D) * 0.05).astype(np.float32),
         'item_bias': (rng.randn(I) * 0.1).astype(np.float32)}
    if bias:
        P['user_bias'] = (rng.randn(U) * 0.1).astype(np.float32)
        P['global_bias'] = np.array([0.3], np.float32)
    st, t = _fused_state(ops, P, 2e-3, 1e-4, B, N + 1, lazy_users=lazy, **kw)
    losses = []
    for s in range(n_steps):
        u = rng.randint(0, U, size=B).astype(np.int64)
        u[:6] = u[6:12]                      # duplicate users inside the batch
        i = rng.randint(0, I, size=(B, N + 1)).astype(np.int64)
        st.step(dev(u), dev(i))
        if s % 10 == 0:
            losses.append(st.last_loss())
    st.flush()
    out = {k: v.cpu().numpy().copy() for k, v in t.items()}
    out.update({'m.' + k: v.cpu().numpy().copy() for k, v in st.m.items() if v is not None})
    out.update({'v.' + k: v.cpu().numpy().copy() for k, v in st.v.items() if v is not None})
    st.check_status()
    return out, losses


def test_lazy_user_adamw_is_bitwise_the_dense_sweep(ops):
    """Exact lazy catch-up == dense AdamW on every user row, across the periodic flush (step 64) boundary."""
    dense, l0 = _run_random_steps(ops, 150, lazy=False)
    lazy, l1 = _run_random_steps(ops, 150, lazy=True)
    assert l0 == l1
    for k in dense:
        assert np.array_equal(dense[k], lazy[k]), k


@pytest.mark.parametrize('D', [33, 130, 402, 512, 640, 1536, 2048])
@pytest.mark.parametrize('opt', ['adamw', 'adam'])
def test_closing_sweep_is_bitwise_the_dense_sweep_over_row_shapes(ops, D, opt):
    """The closing sweep runs one wave per row (k_row_flush_wave) wherever a row fits a wave's registers: every register
    tile (1 / 2 / 4 floats per lane, 1 .. 8 chunks, whole and ragged last chunk) against dense AdamW / Adam with L2 decay
    on every row, every step -- most rows reach the sweep with pending steps (30 steps of 24 out of 500 users)."""
    kw = dict(U=500, I=64, D=D, B=24, N=3, optimizer=opt)
    dense, l0 = _run_random_steps(ops, 30, lazy=False, **kw)
    lazy, l1 = _run_random_steps(ops, 30, lazy=True, **kw)
    assert l0 == l1
    for k in dense:
        assert np.array_equal(dense[k], lazy[k]), (k, D)


@pytest.mark.parametrize('opt', ['adamw', 'adagrad'])
def test_lazy_item_adamw_is_bitwise_the_dense_update(ops, opt):
    """lazy_items: item rows outside the batch keep their zero-gradient steps until they are next touched or flushed --
    bit-identical to updating every item row every step (150 steps: across the flush at 64 and 128), with the touched
    list of each of the three sorts: k_sort_lds (I=3000 items, 48 x 10 entries: most rows untouched), the two-level sort
    (I=900, 1000 x 10 entries) and the block radix sort (I=40, 100 x 12 entries: 30 per item, too dense for k_sort_lds)."""
    for sort, kw in (('lds', dict(U=300, I=3000, D=64, B=48, N=9)), ('two_level', dict(U=120, I=900, D=32, B=1000, N=9)),
                     ('small2', dict(U=300, I=40, D=32, B=100, N=11))):
        assert ops.key_sort_plan(kw['I'], kw['B'] * (kw['N'] + 1), touched=True)['kind'] == sort
        dense, l0 = _run_random_steps(ops, 150, lazy=True, lazy_items=False, optimizer=opt, **kw)
        lazy, l1 = _run_random_steps(ops, 150, lazy=True, lazy_items=True, optimizer=opt, **kw)
        assert l0 == l1
        for k in dense:
            assert np.array_equal(dense[k], lazy[k]), (k, kw)


def test_lazy_items_with_the_device_sampler_and_prefetch(ops):
    """The touched-item list is built by the sort on the side stream (next batch) while the current batch's list is in
    use: same batches, losses and tables as the dense item update."""
    base, b0, l0 = _run_sampled_epoch(ops, overlap=True, hints='right', lazy_items=False)
    lazy, b1, l1 = _run_sampled_epoch(ops, overlap=True, hints='right', lazy_items=True)
    assert l0 == l1
    for k in base:
        assert np.array_equal(base[k], lazy[k]), k


def test_fused_step_is_bitwise_reproducible(ops):
    """No atomics on the data path: two runs of the same batches give identical bits."""
    a, la = _run_random_steps(ops, 40, lazy=True, seed=9, U=80, I=37, B=64, N=30)   # ~50 entries per item
    b, lb = _run_random_steps(ops, 40, lazy=True, seed=9, U=80, I=37, B=64, N=30)
    assert la == lb
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------------
# sampler
# ---------------------------------------------------------------------------------------------------
def _toy_csr(rng, n_users, n_items, dens):
    pairs = np.argwhere(rng.rand(n_users, n_items) < dens)
    return csr_from_pairs(pairs, n_users)


def test_sampler_invariants_and_uniformity(ops, oracle):
    rng = np.random.RandomState(0)
    n_users, n_items, n_neg = 50, 97, 4000
    ptr, idx = _toy_csr(rng, n_users, n_items, 0.3)
    u = np.arange(n_users, dtype=np.int64)
    status = ops.new_status('cuda')
    neg = ops.sample_negatives_uniform(dev(ptr), dev(idx), n_items, dev(u), n_neg, seed=1234, stream_id=5,
                                       status=status).cpu().numpy()
    ops.raise_on_status(status)
    assert neg.shape == (n_users, n_neg)
    assert oracle.count_bad_negatives(ptr, idx, n_items, u, neg) == 0
    # chi-square against the uniform law on each user's complement (df ~ 60-70 -> 99.99% quantile < 130)
    for b in (0, 7, 33):
        allowed = np.setdiff1d(np.arange(n_items), idx[ptr[b]:ptr[b + 1]])
        cnt = np.bincount(neg[b], minlength=n_items)[allowed]
        exp = n_neg / len(allowed)
        chi2 = ((cnt - exp) ** 2 / exp).sum()
        assert chi2 < 2.2 * len(allowed), (b, chi2, len(allowed))
    # with replacement: duplicates exist; reproducible; a different stream gives a different draw
    assert any(len(np.unique(neg[b])) < n_neg for b in range(n_users))
    neg2 = ops.sample_negatives_uniform(dev(ptr), dev(idx), n_items, dev(u), n_neg, seed=1234, stream_id=5).cpu().numpy()
    assert np.array_equal(neg, neg2)
    neg3 = ops.sample_negatives_uniform(dev(ptr), dev(idx), n_items, dev(u), n_neg, seed=1234, stream_id=6).cpu().numpy()
    assert not np.array_equal(neg, neg3)


def test_sampler_same_law_as_reference_style_sampler(ops, oracle):
    """Two-sample check against the numpy restatement of the reference's collate (different RNG, same law)."""
    rng = np.random.RandomState(1)
    n_users, n_items, n_neg = 8, 40, 20000
    ptr, idx = _toy_csr(rng, n_users, n_items, 0.4)
    u = np.arange(n_users, dtype=np.int64)
    a = ops.sample_negatives_uniform(dev(ptr), dev(idx), n_items, dev(u), n_neg, seed=9).cpu().numpy()
    b = oracle.sample_negatives_reference_style(np.random.RandomState(2), ptr, idx, n_items, u, n_neg)
    for r in range(n_users):
        ca = np.bincount(a[r], minlength=n_items).astype(np.float64)
        cb = np.bincount(b[r], minlength=n_items).astype(np.float64)
        assert np.array_equal(ca > 0, cb > 0) or (ca + cb)[(ca > 0) != (cb > 0)].max() < 5
        sel = (ca + cb) > 0
        chi2 = ((ca[sel] - cb[sel]) ** 2 / (ca[sel] + cb[sel])).sum()
        assert chi2 < 2.5 * sel.sum(), (r, chi2, sel.sum())


def test_sampler_user_with_all_items_gives_up(ops):
    n_items = 16
    ptr = np.array([0, n_items], dtype=np.int64)
    idx = np.arange(n_items, dtype=np.int32)
    status = ops.new_status('cuda')
    ops.sample_negatives_uniform(dev(ptr), dev(idx), n_items, dev(np.zeros(1, np.int64)), 3, seed=1, status=status)
    with pytest.raises(RuntimeError):
        ops.raise_on_status(status)


def _run_sampled_epoch(ops, overlap, hints, steps=70, **kw):
    """`steps` device-sampled steps over a fixed interaction order; hints: None | 'right' | 'mixed'."""
    rng = np.random.RandomState(4)
    n_users, n_items, D, B, N = 150, 260, 96, 64, 70     # 64 x 71 entries: above the prefetch minimum (4096)
    pairs = np.argwhere(rng.rand(n_users, n_items) < 0.15)
    pairs = pairs[rng.permutation(len(pairs))]
    assert len(pairs) >= steps * B
    ptr, idx = csr_from_pairs(pairs, n_users)
    P = {'user_emb': (rng.randn(n_users, D) * 0.05).astype(np.float32),
         'item_emb': (rng.randn(n_items, D) * 0.05).astype(np.float32),
         'item_bias': (rng.randn(n_items) * 0.1).astype(np.float32)}
    st, t = _fused_state(ops, P, 1e-3, 1e-4, B, N + 1, seed=5, overlap=overlap, csr_indptr=dev(ptr), csr_indices=dev(idx),
                         coo_user=dev(pairs[:, 0], torch.int32), coo_item=dev(pairs[:, 1], torch.int32), **kw)
    order = torch.from_numpy(np.random.RandomState(6).permutation(len(pairs))).cuda()
    batches, losses = [], []
    for s in range(steps):
        nb = B if s % 7 != 6 else 40                      # ragged batches in between
        if hints and s + 1 < steps:
            nb_next = B if (s + 1) % 7 != 6 else 40
            if hints == 'right' or s % 3 != 1:
                st.hint_next(order, (s + 1) * B, nb_next, N)
            else:
                st.hint_next(order, (s + 5) % steps * B, nb_next, N)   # a wrong guess: must be discarded cleanly
        if hints == 'mixed' and s % 11 == 5:
            u0, i0 = st.last_batch(len(batches[-1][0]), N + 1)   # exactly the rows the previous step wrote
            st.step(u0, i0)                                # an external batch in between also discards the prefetch
            st.hint_next(order, 0, 0, N)
        st.step_sampled(order, s * B, nb, N)
        u, i = st.last_batch(nb, N + 1)
        batches.append((u.cpu().numpy(), i.cpu().numpy()))
        losses.append(st.last_loss())
    st.flush()
    st.check_status()
    out = {k: v.cpu().numpy().copy() for k, v in t.items()}
    out.update({'m.' + k: v.cpu().numpy().copy() for k, v in st.m.items() if v is not None})
    return out, batches, losses


def test_prefetched_batches_change_nothing(ops):
    """hsk_bprmf_hint_next: batches sampled + sorted one step ahead on the side stream give the same batches, losses
    and parameters, bit for bit, as the inline sequence -- also across the flush boundary (step 64)."""
    base, b0, l0 = _run_sampled_epoch(ops, overlap=False, hints=None)
    pref, b1, l1 = _run_sampled_epoch(ops, overlap=True, hints='right')
    assert l0 == l1
    for (u0, i0), (u1, i1) in zip(b0, b1):
        assert np.array_equal(u0, u1) and np.array_equal(i0, i1)
    for k in base:
        assert np.array_equal(base[k], pref[k]), k


@pytest.mark.parametrize('shape', [
    # (n_users, n_items, D, B, N, lazy_users, steps in the first / second chunked call)
    (150, 260, 96, 64, 70, True, 40, 30),        # below the graph chunk: eager launches from C
    (300, 400, 402, 128, 50, False, 150, 75),    # BASELINE configs[1] row / batch shape, dense user sweep: replayed graphs
    (300, 400, 402, 128, 50, True, 150, 75),     # the same with the lazy user AdamW (flush after every replayed run)
    (200, 500, 64, 128, 1, False, 200, 25),      # BASELINE configs[0] row / batch shape (one negative: 256 entries)
    (900, 700, 128, 2048, 10, True, 70, 66),     # a batch large enough for the late fork + four-kernel sort in the graph
])
def test_multi_step_call_equals_single_steps(ops, shape):
    """hsk_bprmf_train_steps (the epoch's inner loop issued from C; runs of 64 steps as replayed HIP graphs whose
    kernels read the batch offset / step index from a device descriptor) == the same steps issued one by one from the
    host, bit for bit: parameters, moments and the loss sum."""
    n_users, n_items, D, B, N, lazy, n1, n2 = shape
    rng = np.random.RandomState(4)
    pairs = np.argwhere(rng.rand(n_users, n_items) < 0.15)
    pairs = pairs[rng.permutation(len(pairs))]
    ptr, idx = csr_from_pairs(pairs, n_users)
    P = {'user_emb': (rng.randn(n_users, D) * 0.05).astype(np.float32),
         'item_emb': (rng.randn(n_items, D) * 0.05).astype(np.float32),
         'item_bias': (rng.randn(n_items) * 0.1).astype(np.float32)}
    n_pos = len(pairs)
    reps = -(-(n1 + n2) * B // n_pos)
    order = torch.from_numpy(np.concatenate([np.random.RandomState(6 + r).permutation(n_pos) for r in range(reps)])).cuda()
    res = []
    for chunked in (False, True):
        st, t = _fused_state(ops, P, 1e-3, 1e-4, B, N + 1, seed=5, csr_indptr=dev(ptr), csr_indices=dev(idx),
                             coo_user=dev(pairs[:, 0], torch.int32), coo_item=dev(pairs[:, 1], torch.int32),
                             lazy_users=lazy)
        st.st.nnz = order.numel()      # the run walks `order`, which repeats the interactions
        if chunked:
            st.steps_sampled(order, 0, n1, B, N)
            st.step_sampled(order, n1 * B, B, N)             # an eager step between two replayed runs
            st.steps_sampled(order, (n1 + 1) * B, n2 - 1, B, N)
        else:
            for s in range(n1 + n2):
                st.step_sampled(order, s * B, B, N)
        st.flush()
        st.check_status()
        assert st.step_count == n1 + n2
        # the chunked run really went through the graphs: every full run of 64 steps inside the two calls
        assert st.graph_replays() == ((n1 // 64 + (n2 - 1) // 64) if chunked else 0)
        mom = {'m_' + k: v.cpu().numpy().copy() for k, v in st.m.items() if v is not None}
        mom.update({'v_' + k: v.cpu().numpy().copy() for k, v in st.v.items() if v is not None})
        res.append(({k: v.cpu().numpy().copy() for k, v in t.items()}, mom, st.pop_loss_sum()))
    assert res[0][2] == res[1][2]
    for k in res[0][0]:
        assert np.array_equal(res[0][0][k], res[1][0][k]), k
    for k in res[0][1]:
        assert np.array_equal(res[0][1][k], res[1][1][k]), k


@pytest.mark.parametrize('n_steps', [6, 7, 8])
def test_last_batch_after_a_flush_of_a_pipelined_run(ops, n_steps):
    """hsk_bprmf_last_batch after a flush returns the batch of the last step whichever of the pipeline's three buffer sets
    it sat in (the flush folds the running set index back into {0, 1}; found by tools/stress_pipeline.py)."""
    n_users, n_items, D, B, N = 500, 6000, 256, 2048, 17
    rng = np.random.RandomState(4)
    pairs = np.argwhere(rng.rand(n_users, n_items) < 0.02)
    pairs = pairs[rng.permutation(len(pairs))]
    ptr, idx = csr_from_pairs(pairs, n_users)
    P = {'user_emb': (rng.randn(n_users, D) * 0.05).astype(np.float32),
         'item_emb': (rng.randn(n_items, D) * 0.05).astype(np.float32),
         'item_bias': (rng.randn(n_items) * 0.1).astype(np.float32)}
    order = torch.from_numpy(rng.permutation(len(pairs))).cuda()
    lib = ops._lib.load()
    got = []
    try:
        for pipelined in (True, False):
            lib.hsk_bprmf_set_pipeline(1 if pipelined else 0)
            st, t = _fused_state(ops, P, 1e-3, 1e-4, B, N + 1, seed=5, csr_indptr=dev(ptr), csr_indices=dev(idx),
                                 coo_user=dev(pairs[:, 0], torch.int32), coo_item=dev(pairs[:, 1], torch.int32))
            st.hint_after_run(order, n_steps * B, B, N, n_batches=2)
            st.steps_sampled(order, 0, n_steps, B, N)
            st.flush()
            bu, bi = st.last_batch(B, N + 1)
            got.append((bu.cpu().numpy(), bi.cpu().numpy()))
    finally:
        lib.hsk_bprmf_set_pipeline(1)
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    assert np.array_equal(got[0][0], pairs[order.cpu().numpy()[(n_steps - 1) * B: n_steps * B], 0])


def test_large_batch_at_dim_768_takes_the_unpartitioned_forward(ops):
    """D = 768 is a multiple of 256 but not a whole number of the partitioned kernel's chunk counts (1, 2, 4, 8): a large
    batch on a mid-size item table must fall back to the un-partitioned forward, not fail (found by
    tools/stress_pipeline.py: 'item-partitioned forward selected for dim 768')."""
    n_users, n_items, D, B, N = 300, 4000, 768, 2048, 17          # item table 12.3 MB: the partition rule's range
    rng = np.random.RandomState(2)
    pairs = np.argwhere(rng.rand(n_users, n_items) < 0.02)
    pairs = pairs[rng.permutation(len(pairs))]
    ptr, idx = csr_from_pairs(pairs, n_users)
    P = {'user_emb': (rng.randn(n_users, D) * 0.05).astype(np.float32),
         'item_emb': (rng.randn(n_items, D) * 0.05).astype(np.float32),
         'item_bias': (rng.randn(n_items) * 0.1).astype(np.float32)}
    order = torch.from_numpy(rng.permutation(len(pairs))).cuda()
    st, t = _fused_state(ops, P, 1e-3, 1e-4, B, N + 1, seed=5, csr_indptr=dev(ptr), csr_indices=dev(idx),
                         coo_user=dev(pairs[:, 0], torch.int32), coo_item=dev(pairs[:, 1], torch.int32))
    assert st.batch_columns(B, N + 1) == N + 1
    st.steps_sampled(order, 0, 3, B, N)
    st.flush()
    st.check_status()
    assert np.isfinite(st.last_loss()) and st.pipelined_steps() == 0
    assert np.isfinite(t['item_emb'].cpu().numpy()).all()


@pytest.mark.parametrize('lazy,shape', [(True, 'narrow'), (False, 'narrow'), (True, 'wide'), (False, 'narrow-popular')])
def test_in_launch_pipeline_equals_side_stream_prefetch(ops, lazy, shape):
    """Large batches on the item-partitioned forward prepare the next two batches INSIDE the step's own launches (sampler
    and the item sort's phases as extra workgroups of the forward / item-user kernels, csrc/hsk_fused.hip: hsk_pipe_step)
    instead of five launches on a side stream.  Same draws, same sort, same arithmetic: tables, moments and losses equal
    the side-stream path's bit for bit -- across runs chained by hint_after_run (two batches named, one, none, a WRONG
    one), a single step issued through the other path in between, and a flush in the middle.
    narrow: 6000 items -- the riding sampler tests membership in an LDS bitmap; user 0 has > 256 positives (beyond the
    prefetched registers).  wide: 40 000 items (no bitmap: the staged binary search), rows of ~400 positives, user 0 with
    > 1024 (searched in global memory).  narrow-popular: the `popular` strategy (alias table) through the riding sampler."""
    popular = shape.endswith('popular')
    shape = shape.split('-')[0]
    if shape == 'narrow':
        n_users, n_items, D, B, N, dens, n_part = 700, 6000, 256, 2048, 17, 0.02, 2
    else:
        n_users, n_items, D, B, N, dens, n_part = 300, 40000, 256, 2048, 17, 0.01, 2   # (8 by size, 2 left by n_neg >= 8 P)
    rng = np.random.RandomState(9)
    mask = rng.rand(n_users, n_items) < dens
    mask[0] = rng.rand(n_items) < (0.1 if shape == 'narrow' else 0.03)   # 600 / 1200 positives
    pairs = np.argwhere(mask)
    pairs = pairs[rng.permutation(len(pairs))]
    ptr, idx = csr_from_pairs(pairs, n_users)
    P = {'user_emb': (rng.randn(n_users, D) * 0.05).astype(np.float32),
         'item_emb': (rng.randn(n_items, D) * 0.05).astype(np.float32),
         'item_bias': (rng.randn(n_items) * 0.1).astype(np.float32)}
    n_pos = len(pairs)
    n_total = 40
    reps = -(-(n_total + 4) * B // n_pos)
    order = torch.from_numpy(np.concatenate([np.random.RandomState(6 + r).permutation(n_pos) for r in range(reps)])).cuda()
    lib = ops._lib.load()
    res = []
    try:
        for pipelined in (True, False):
            lib.hsk_bprmf_set_pipeline(1 if pipelined else 0)
            alias = None
            if popular:
                pr, al = ops.build_alias_table(np.bincount(pairs[:, 1], minlength=n_items).astype(np.float64) ** 0.75 + 1e-3)
                alias = (dev(pr), dev(al))
            st, t = _fused_state(ops, P, 1e-3, 1e-4, B, N + 1, seed=5, csr_indptr=dev(ptr), csr_indices=dev(idx),
                                 coo_user=dev(pairs[:, 0], torch.int32), coo_item=dev(pairs[:, 1], torch.int32),
                                 lazy_users=lazy, alias=alias)
            st.st.nnz = order.numel()
            assert st.batch_columns(B, N + 1) == N + n_part   # the partitioned forward: the shape the pipeline is for
            s = 0
            st.hint_after_run(order, 7 * B, B, N, n_batches=2)
            st.steps_sampled(order, s * B, 7, B, N); s += 7   # cold start, tail: two batches named
            st.hint_after_run(order, 12 * B, B, N, n_batches=1)
            st.steps_sampled(order, s * B, 5, B, N); s += 5   # continues on prepared batches; tail: one batch
            st.steps_sampled(order, s * B, 3, B, N); s += 3   # tail: none
            st.hint_after_run(order, 33 * B, B, N, n_batches=2)   # a WRONG guess: the next run starts elsewhere
            st.steps_sampled(order, s * B, 4, B, N); s += 4
            st.step_sampled(order, s * B, B, N); s += 1       # one step through the single-step path
            st.hint_after_run(order, (s + 6) * B, B, N, n_batches=2)
            st.steps_sampled(order, s * B, 6, B, N); s += 6
            st.flush()                                        # drops the two prepared batches
            losses_mid = st.pop_loss_sum()
            st.steps_sampled(order, s * B, n_total - s, B, N)
            st.flush()
            st.check_status()
            assert st.step_count == n_total
            assert (st.pipelined_steps() == n_total - 1) if pipelined else (st.pipelined_steps() == 0)
            mom = {'m_' + k: v.cpu().numpy().copy() for k, v in st.m.items() if v is not None}
            mom.update({'v_' + k: v.cpu().numpy().copy() for k, v in st.v.items() if v is not None})
            bu, bi = st.last_batch(B, N + 1)
            res.append(({k: v.cpu().numpy().copy() for k, v in t.items()}, mom, (losses_mid, st.pop_loss_sum()),
                        (bu.cpu().numpy(), bi.cpu().numpy())))
    finally:
        lib.hsk_bprmf_set_pipeline(1)
    assert res[0][2] == res[1][2]
    assert np.array_equal(res[0][3][0], res[1][3][0]) and np.array_equal(res[0][3][1], res[1][3][1])
    for k in res[0][0]:
        assert np.array_equal(res[0][0][k], res[1][0][k]), k
    for k in res[0][1]:
        assert np.array_equal(res[0][1][k], res[1][1][k]), k


@pytest.mark.parametrize('shape', [
    # (n_users, n_items, D, B, K, popular, sort): which of the item sorts the step picks (hip_ops.key_sort_plan's name)
    (300, 3706, 32, 128, 51, False, 'lds'),     # k_sort_lds: <= 8192 entries, <= 4 per item on average (BASELINE configs[1] shape)
    (300, 1682, 32, 128, 2, False, 'lds'),      # k_sort_lds, 256 entries (BASELINE configs[0] shape)
    (300, 40, 32, 100, 12, False, 'small2'),    # k_sort_lds is not eligible (30 entries per item): block radix sort
    (300, 2000, 32, 64, 101, True, 'lds'),      # k_sort_lds with popular items: lists far longer than 8 entries (wave rank pass)
    (300, 5000, 32, 1024, 33, False, 'two_level'),   # > 8192 entries: the four-kernel two-level sort
    (300, 5000, 32, 1024, 33, True, 'two_level'),    # ... with lists of thousands of entries
    (300, 6000, 256, 2048, 17, True, 'two_level'),   # item-partitioned forward (P = 2): rows of K + P - 1 columns
    (300, 500, 32, 128, 16, False, 'small2'),   # 2048 entries: k_sort_small<2> with every thread full (no padding key)
    (300, 1000, 32, 128, 32, False, 'small4'),  # 4096 entries: k_sort_small<4>, no padding key
    (300, 2047, 32, 128, 64, False, 'small8'),  # 8192 entries: k_sort_small<8>, no padding key
    (300, 8000, 32, 128, 64, False, 'lds'),     # k_sort_lds at its largest: 8000 items, 8192 entries, 161 792 B of LDS
])
def test_item_sort_is_the_stable_sort_by_item(ops, shape):
    """perm / offsets of the step's batch == numpy's stable argsort of the item ids, whichever kernel built them."""
    n_users, n_items, D, B, K, popular, sort = shape
    rng = np.random.RandomState(11)
    P = {'user_emb': (rng.randn(n_users, D) * 0.05).astype(np.float32),
         'item_emb': (rng.randn(n_items, D) * 0.05).astype(np.float32)}
    st, _ = _fused_state(ops, P, 1e-3, 0.0, B, K)
    u = rng.randint(0, n_users, size=B).astype(np.int64)
    i = rng.randint(0, n_items, size=(B, K)).astype(np.int64)
    if popular:                                # a few very popular items
        i[rng.rand(B, K) < 0.3] = 3
        i[:, 0] = 7
    st.step(dev(u), dev(i))
    cols = st.batch_columns(B, K)              # the partitioned layout repeats the positive
    if D == 256:
        assert cols == K + 1
    else:
        assert cols == K
    assert ops.key_sort_plan(n_items, B * cols)['kind'] == sort
    # partitioned rows: the positive, cols - K columns that are no entries (the sort skips them), the negatives
    i = np.concatenate([i[:, :1], np.full((B, cols - K), -1, dtype=np.int64), i[:, 1:]], axis=1)
    flat = i.reshape(-1)
    n_ent = int((flat >= 0).sum())
    perm, offs = (x.cpu().numpy() for x in st.last_sort(B * cols))
    want = np.argsort(np.where(flat < 0, n_items, flat), kind='stable')[:n_ent]
    assert np.array_equal(perm[:n_ent], want)
    flat = flat[flat >= 0]
    assert np.array_equal(offs, np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=n_items))]))
    st.check_status()


def test_wrong_hints_are_discarded(ops):
    """A hint that does not match the next call (or is followed by an external batch) costs time, never results."""
    base, b0, l0 = _run_sampled_epoch(ops, overlap=True, hints=None)
    mixed_ref, _, _ = _run_sampled_epoch(ops, overlap=False, hints='mixed')     # hints are no-ops without overlap
    mixed, _, _ = _run_sampled_epoch(ops, overlap=True, hints='mixed')
    for k in mixed:
        assert np.array_equal(mixed[k], mixed_ref[k]), k
    plain, b1, l1 = _run_sampled_epoch(ops, overlap=False, hints=None)
    assert l0 == l1
    for k in base:
        assert np.array_equal(base[k], plain[k]), k


def test_fused_sampled_step_matches_oracle_on_its_own_batch(ops, oracle):
    """Device-built batch: read back (u, i) the step used, check sampler invariants, replay in the oracle."""
    rng = np.random.RandomState(3)
    n_users, n_items, D, B, N = 120, 300, 64, 96, 20
    pairs = np.argwhere(rng.rand(n_users, n_items) < 0.05)
    pairs = pairs[rng.permutation(len(pairs))]
    ptr, idx = csr_from_pairs(pairs, n_users)
    P = {'user_emb': (rng.randn(n_users, D) * 0.05).astype(np.float32),
         'item_emb': (rng.randn(n_items, D) * 0.05).astype(np.float32),
         'item_bias': (rng.randn(n_items) * 0.1).astype(np.float32)}
    st, t = _fused_state(ops, P, 1e-3, 1e-4, B, N + 1, seed=77, csr_indptr=dev(ptr), csr_indices=dev(idx),
                         coo_user=dev(pairs[:, 0], torch.int32), coo_item=dev(pairs[:, 1], torch.int32))
    tr = oracle.MfOracleTrainer(P['user_emb'], P['item_emb'], P['item_bias'], lr=1e-3, wd=1e-4)
    order = torch.randperm(len(pairs), device='cuda')
    prev = None
    for s in range(3):
        nb = B if s < 2 else 40  # ragged tail
        st.step_sampled(order, s * B, nb, N)
        u, i = st.last_batch(nb, N + 1)
        u, i = u.cpu().numpy(), i.cpu().numpy()
        sel = order[s * B:s * B + nb].cpu().numpy()
        assert np.array_equal(u, pairs[sel, 0]) and np.array_equal(i[:, 0], pairs[sel, 1])
        assert oracle.count_bad_negatives(ptr, idx, n_items, u, i[:, 1:]) == 0
        if prev is not None:
            assert not np.array_equal(prev, i[:40, 1:])  # fresh negatives every step
        prev = i[:40, 1:].copy()
        loss_ref, _, _, _ = tr.step(u, i)
        assert abs(st.last_loss() - loss_ref) <= 1e-6 * loss_ref
    st.flush()
    for name in P:
        assert_adam_param_close(t[name].cpu().numpy(), tr.P[name], name)
    st.check_status()


# ---------------------------------------------------------------------------------------------------
# evaluation
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('split', ['val', 'test'])
def test_eval_topk_metrics_vs_golden(ops, split):
    fx = load_golden('g3_eval.npz')
    U, I = dev(fx['param.user_embeddings.weight']), dev(fx['param.item_embeddings.weight'])
    Ib, Ub = dev(fx['param.item_bias.weight'].reshape(-1)), dev(fx['param.user_bias.weight'].reshape(-1))
    gb = dev(fx['param.global_bias'])
    n_users = int(fx['n_users'])
    excl = fx['train'] if split == 'val' else np.concatenate([fx['train'], fx['val']])
    e_ptr, e_idx = csr_from_pairs(excl, n_users)
    l_ptr, l_idx = csr_from_pairs(fx[split], n_users)
    u = fx[f'{split}.u']
    status = ops.new_status('cuda')
    vals, ids, scores = ops.mf_eval_topk(U, I, Ib, Ub, gb, dev(u), 100, dev(e_ptr), dev(e_idx), status=status,
                                         want_scores=True)
    ops.raise_on_status(status)
    sc, ref = scores.cpu().numpy(), fx[f'{split}.masked_logits']
    assert np.array_equal(np.isinf(sc), np.isinf(ref))
    fin = ~np.isinf(ref)
    np.testing.assert_allclose(sc[fin], ref[fin], rtol=RTOL, atol=2e-6)
    ids = ids.cpu().numpy()
    ref_ids = fx[f'{split}.top100']
    # same ranking except where two scores differ by less than fp32 rounding of the dot product
    mism = ids != ref_ids
    if mism.any():
        r, c = np.nonzero(mism)
        assert np.abs(ref[r, ids[r, c]] - ref[r, ref_ids[r, c]]).max() < 2e-6
    assert mism.mean() < 0.01
    assert np.all(np.diff(vals.cpu().numpy(), axis=1) <= 0)
    ks = [5, 10, 50, 100]
    met = ops.rank_metrics(ids_t := torch.from_numpy(ids).cuda(), dev(u), dev(l_ptr), dev(l_idx), ks).cpu().numpy()
    del ids_t
    names = [str(x) for x in fx[f'{split}.metric_names']]
    got = {}
    grp = fx['user_group'][u]
    for t, k in enumerate(ks):
        for j, nm in enumerate(('precision', 'recall', 'ndcg')):
            got[f'{nm}@{k}'] = met[:, t, j].astype(np.float64).mean()
            for g in (0, 1):
                got[f'group_{g}_{nm}@{k}'] = met[grp == g, t, j].astype(np.float64).mean()
    for name, val in zip(names, fx[f'{split}.metric_values']):
        assert abs(got[name] - val) <= 1e-6 + 1e-4 * abs(val), name


@pytest.mark.parametrize('fused', [False, True])
def test_eval_d512_wide_catalogue_vs_golden(ops, fused):
    """G3 at D = 512 over 4224 items from the reference: the VEC4 GEMM at the BASELINE embedding size with the two-pass
    wide-row top-k (materialised path) and with the selection inside the GEMM (fused path)."""
    from conftest import g3_d512_params
    fx = load_golden('g3_eval_d512.npz')
    Un, In, Ibn = g3_d512_params(fx)
    U, I, Ib = dev(Un), dev(In), dev(Ibn)
    n_users = int(fx['n_users'])
    e_ptr, e_idx = csr_from_pairs(fx['train'], n_users)
    l_ptr, l_idx = csr_from_pairs(fx['val'], n_users)
    u = fx['val.u']
    vals, ids, scores = ops.mf_eval_topk(U, I, Ib, None, None, dev(u), 100, dev(e_ptr), dev(e_idx),
                                         want_scores=not fused)
    ref = fx['val.masked_logits']
    if not fused:
        sc = scores.cpu().numpy()
        assert np.array_equal(np.isinf(sc), np.isinf(ref))
        fin = ~np.isinf(ref)
        np.testing.assert_allclose(sc[fin], ref[fin], rtol=RTOL, atol=2e-6 * np.abs(ref[fin]).max())
    ids = ids.cpu().numpy()
    ref_ids = fx['val.top100']
    mism = ids != ref_ids
    if mism.any():   # the same ranking except where two scores differ by less than fp32 rounding of the dot product
        r, c = np.nonzero(mism)
        assert np.abs(ref[r, ids[r, c]] - ref[r, ref_ids[r, c]]).max() < 2e-6 * np.abs(ref[np.isfinite(ref)]).max()
    assert mism.mean() < 0.01
    got_vals = vals.cpu().numpy()
    np.testing.assert_allclose(got_vals, np.take_along_axis(ref, ids, axis=1), rtol=RTOL,
                               atol=2e-6 * np.abs(ref[np.isfinite(ref)]).max())
    ks = [5, 10, 50, 100]
    met = ops.rank_metrics(torch.from_numpy(ids).cuda(), dev(u), dev(l_ptr), dev(l_idx), ks).cpu().numpy()
    got = {}
    grp = fx['user_group'][u]
    for t, k in enumerate(ks):
        for j, nm in enumerate(('precision', 'recall', 'ndcg')):
            got[f'{nm}@{k}'] = met[:, t, j].astype(np.float64).mean()
            for g in (0, 1):
                got[f'group_{g}_{nm}@{k}'] = met[grp == g, t, j].astype(np.float64).mean()
    for name, val in zip([str(x) for x in fx['val.metric_names']], fx['val.metric_values']):
        assert abs(got[name] - val) <= 1e-6 + 1e-4 * abs(val), name


@pytest.mark.parametrize('shape', [
    # (rows, n_users, n_items, D, k)
    (300, 300, 5000, 512, 100),      # D = 512 (BASELINE configs[2-3]), several item splits + the split merge
    (130, 200, 1000, 30, 100),       # D % 4 != 0: scalar staging loads; one split of 8 tiles
    (70, 70, 40000, 64, 100),        # long rows: thresholds, appends and repeated compactions
    (257, 400, 300, 128, 5),         # small k, three row blocks (the last one ragged)
    (64, 64, 129, 16, 100),          # two tiles, the second with a single column
])
def test_fused_topk_equals_materialised_topk(ops, shape):
    """Top-k selected inside the score GEMM (no score matrix) == top-k of the materialised, masked score matrix:
    same values, same ids, same order -- with biases, exclusions (one user with fewer than k admissible items: the
    -inf entries fill up, lowest id first), exact ties (duplicated item rows) and an item range."""
    R, n_users, n_items, D, k = shape
    # both kernels follow the same arithmetic switch and the same order of operations: bit-equal in every form (form 2,
    # the fp16-pair core, runs wherever the rows are 16-byte aligned -- both paths then take the 256 x 256 kernels -- and
    # both fall back to form 1 together where they are not: D = 30)
    try:
        for form in (ops.EVAL_ARITH_FP32, ops.EVAL_ARITH_BF16X3, ops.EVAL_ARITH_F16X2):
            ops.set_eval_arith(form)
            _fused_vs_materialised(ops, R, n_users, n_items, D, k, cross=False)
    finally:
        ops.set_eval_arith(ops.EVAL_ARITH_DEFAULT)
    # the forms against each other (materialised exact-fp32 vs fused in the default form): values to 4e-6 of the largest
    # score, ids wherever neighbouring scores are clearly further apart than that
    _fused_vs_materialised(ops, R, n_users, n_items, D, k, cross=True)


@pytest.mark.parametrize('shape', [(300, 300, 5000, 512, 100), (257, 400, 1300, 128, 5), (64, 64, 129, 16, 100),
                                   # 28 x 28 block tiles of 256 x 256: the materialised path takes k_score_gemm_x3_wide (one
                                   # wave per SIMD, hand-interleaved k-steps); ragged in rows, items and K (200 -> 224)
                                   (7000, 400, 7100, 200, 100)])
def test_presplit_operands_equal_in_loop_split(ops, shape):
    """The score GEMMs fed from the pre-pass that cuts the operands into their bf16 pieces once per call
    (hsk_mf_eval_topk_planes / a hsk_mf_eval_fused_ws_bytes_dim workspace) return the very bits of the form that splits
    every tile in its loop (no scratch given): scores, top-k values, ids -- materialised and fused, whole catalogue and an
    item range with a ragged last tile."""
    R, n_users, n_items, D, k = shape
    g = torch.Generator(device='cuda').manual_seed(11)
    U = torch.randn(n_users, D, device='cuda', generator=g) * 0.3
    I = torch.randn(n_items, D, device='cuda', generator=g) * 0.3
    Ib = torch.randn(n_items, device='cuda', generator=g) * 0.1
    rng = np.random.RandomState(3)
    pairs = np.argwhere(rng.rand(n_users, n_items) < min(0.05, 200.0 / n_items))
    e_ptr, e_idx = csr_from_pairs(pairs, n_users)
    u = torch.from_numpy(rng.randint(0, n_users, size=R).astype(np.int64)).cuda()
    ops.set_eval_arith(ops.EVAL_ARITH_BF16X3)   # (form 2 exists only on pre-split operands: test_f16_pair_scores_...)
    try:
        for lo, cnt in ((0, n_items), (n_items // 3, n_items - n_items // 3 - 7)):
            kk = min(k, cnt)
            for want in (True, False):
                a = ops.mf_eval_topk(U, I, Ib, None, None, u, kk, dev(e_ptr), dev(e_idx), item_begin=lo, item_count=cnt,
                                     want_scores=want, presplit=True)
                b = ops.mf_eval_topk(U, I, Ib, None, None, u, kk, dev(e_ptr), dev(e_idx), item_begin=lo, item_count=cnt,
                                     want_scores=want, presplit=False)
                assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)), (shape, lo, want)
                assert torch.equal(a[1], b[1]), (shape, lo, want)
                if want:
                    assert torch.equal(a[2][:R * cnt].view(torch.int32), b[2][:R * cnt].view(torch.int32))
    finally:
        ops.set_eval_arith(ops.EVAL_ARITH_DEFAULT)


@pytest.mark.parametrize('case', ['init-scale', 'wide-range', 'tiny', 'huge', 'zeros-and-inf', 'ragged-k'])
def test_f16_pair_scores_against_float64(ops, case):
    """Form 2 of the score arithmetic (two fp16 pieces per operand at a power-of-two scale taken from the table's largest
    |x|, three products: csrc/hsk_gemm_wide_h2.h) against float64 on the same fp32 tables, beside the exact-fp32 MFMA form:
    its error stays within 4x the fp32 form's own (both are dominated by the fp32 accumulation; measured 0.8-2x) and far inside north_star's
    1e-5 of the largest score -- for tables at the reference's init scale (std 0.1 / D), with per-column scales spread over
    three decades, with magnitudes near the ends of the fp32 range, and with zero rows / an infinite entry."""
    R, n_users, n_items, D = 300, 300, 3000, (200 if case == 'ragged-k' else 128)   # 200 -> seven k-steps of 32, the last ragged
    g = torch.Generator(device='cuda').manual_seed(23)
    U = torch.randn(n_users, D, device='cuda', generator=g)
    I = torch.randn(n_items, D, device='cuda', generator=g)
    if case == 'init-scale':
        U, I = U * (0.1 / D), I * (0.1 / D)
    elif case == 'wide-range':
        cs = torch.exp(torch.randn(D, device='cuda', generator=g) * 2.3)
        U, I = U * cs, I * cs
    elif case == 'tiny':
        U, I = U * 1e-17, I * 1e-15
    elif case == 'huge':
        U, I = U * 3e12, I * 1e14
    elif case == 'ragged-k':
        U, I = U * 0.3, I * 0.3
    else:
        U[5] = 0.0
        I[7] = 0.0
        I[11, 3] = float('inf')
    u = torch.arange(R, device='cuda', dtype=torch.int64)
    out = {}
    try:
        for form in (ops.EVAL_ARITH_FP32, ops.EVAL_ARITH_F16X2):
            ops.set_eval_arith(form)
            out[form] = ops.mf_eval_topk(U, I, None, None, None, u, 10, want_scores=True)[2][:R * n_items].view(R, n_items).double()
    finally:
        ops.set_eval_arith(ops.EVAL_ARITH_DEFAULT)
    ref = U.double() @ I.double().T
    fin = torch.isfinite(ref)
    scale = ref[fin].abs().max().item()
    err = {f: ((o - ref)[fin].abs().max().item()) for f, o in out.items()}
    assert err[ops.EVAL_ARITH_F16X2] <= max(4.0 * err[ops.EVAL_ARITH_FP32], 5e-7 * scale), (case, err, scale)
    assert err[ops.EVAL_ARITH_F16X2] <= 2e-6 * scale, (case, err, scale)
    if case == 'zeros-and-inf':   # the infinite entry: nothing finite in its column (inf or nan, as in fp32); zero row: zeros
        assert not torch.isfinite(out[ops.EVAL_ARITH_F16X2][:, 11]).any()
        assert (out[ops.EVAL_ARITH_F16X2][5][fin[5]] == 0).all()


def _fused_vs_materialised(ops, R, n_users, n_items, D, k, cross):
    exact = not cross

    def arith(materialised):   # cross: the materialised reference in exact fp32, the fused path in the default form
        if cross:
            ops.set_eval_arith(ops.EVAL_ARITH_FP32 if materialised else ops.EVAL_ARITH_DEFAULT)

    g = torch.Generator(device='cuda').manual_seed(7)
    U = torch.randn(n_users, D, device='cuda', generator=g) * 0.3
    I = torch.randn(n_items, D, device='cuda', generator=g) * 0.3
    I[n_items // 2: n_items // 2 + 20] = I[:20]              # exact ties between items far apart
    Ib = torch.randn(n_items, device='cuda', generator=g) * 0.1
    Ib[n_items // 2: n_items // 2 + 20] = Ib[:20]
    Ub = torch.randn(n_users, device='cuda', generator=g) * 0.1
    gb = torch.tensor([0.3], device='cuda')
    rng = np.random.RandomState(5)
    pairs = np.argwhere(rng.rand(n_users, n_items) < min(0.05, 300.0 / n_items))
    if n_items > k:       # user 1 keeps only k - 30 admissible items
        keep = rng.choice(n_items, size=max(k - 30, 1), replace=False)
        rest = np.setdiff1d(np.arange(n_items), keep)
        pairs = np.concatenate([pairs[pairs[:, 0] != 1], np.stack([np.ones_like(rest), rest], axis=1)])
    e_ptr, e_idx = csr_from_pairs(pairs, n_users)
    u = torch.from_numpy(rng.randint(0, n_users, size=R).astype(np.int64)).cuda()
    u[0] = 1
    for lo, cnt in ((0, n_items), (n_items // 3, n_items - n_items // 3 - 7)):
        kk = min(k, cnt)
        arith(True)
        v_ref, i_ref, sc = ops.mf_eval_topk(U, I, Ib, Ub, gb, u, kk, dev(e_ptr), dev(e_idx), item_begin=lo,
                                            item_count=cnt, want_scores=True)
        arith(False)
        v, i, none = ops.mf_eval_topk(U, I, Ib, Ub, gb, u, kk, dev(e_ptr), dev(e_idx), item_begin=lo, item_count=cnt,
                                      want_scores=False)
        assert none is None and sc is not None
        _same_topk(v, i, v_ref, i_ref, exact, (lo, cnt))
    # without an exclusion CSR and without biases
    arith(True)
    v_ref, i_ref, _ = ops.mf_eval_topk(U, I, None, None, None, u, min(k, n_items), want_scores=True)
    arith(False)
    v, i, _ = ops.mf_eval_topk(U, I, None, None, None, u, min(k, n_items), want_scores=False)
    _same_topk(v, i, v_ref, i_ref, exact, 'plain')


def _same_topk(v, i, v_ref, i_ref, exact, what):
    if exact:
        assert torch.equal(i, i_ref), (what, int((i != i_ref).sum()))
        assert torch.equal(v, v_ref), what
        return
    fin = torch.isfinite(v_ref)
    assert torch.equal(torch.isfinite(v), fin), what
    scale = float(v_ref[fin].abs().max())
    assert float((v[fin] - v_ref[fin]).abs().max()) <= 4e-6 * scale, what   # two fp32-accurate sums of up to 512 terms
    # positions whose reference score is clear of both neighbours (ties and near-ties may swap between the two forms)
    d = (v_ref[:, :-1] - v_ref[:, 1:]).abs() > 1.6e-5 * scale
    clear = torch.ones_like(v_ref, dtype=torch.bool)
    clear[:, :-1] &= d
    clear[:, 1:] &= d
    clear &= fin
    assert clear.float().mean() > 0.5, what
    assert torch.equal(i[clear], i_ref[clear]), what


def test_eval_item_shards_merge_to_global_topk(ops):
    """Item-sharded scoring + hsk_topk_merge == un-sharded top-k (the multi-GPU eval path on one device)."""
    torch.manual_seed(0)
    n_users, n_items, D, k = 70, 1000, 128, 100
    U, I = torch.randn(n_users, D, device='cuda'), torch.randn(n_items, D, device='cuda')
    Ib = torch.randn(n_items, device='cuda')
    rng = np.random.RandomState(5)
    e_ptr, e_idx = _toy_csr(rng, n_users, n_items, 0.1)
    u = torch.arange(n_users, device='cuda')
    v0, i0, _ = ops.mf_eval_topk(U, I, Ib, None, None, u, k, dev(e_ptr), dev(e_idx))
    parts_v, parts_i = [], []
    bounds = [0, 130, 400, 401, 777, 1000]  # uneven shards, one of them smaller than k
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        kk = min(k, hi - lo)
        v, i, _ = ops.mf_eval_topk(U, I, Ib, None, None, u, kk, dev(e_ptr), dev(e_idx), item_begin=lo, item_count=hi - lo)
        pad_v = torch.full((n_users, k), float('-inf'), device='cuda')
        pad_i = torch.full((n_users, k), 2 ** 31 - 1, dtype=torch.int32, device='cuda')
        pad_v[:, :kk], pad_i[:, :kk] = v, i
        parts_v.append(pad_v)
        parts_i.append(pad_i)
    mv, mi = ops.topk_merge(torch.stack(parts_v).contiguous(), torch.stack(parts_i).contiguous())
    assert torch.equal(mi, i0) and torch.equal(mv, v0)


def test_topk_dense_ties_and_neg_inf(ops, oracle):
    x = torch.zeros(5, 300, device='cuda')
    x[0] = torch.arange(300, 0, -1)
    x[1, :] = 1.0                       # all tied -> lowest indices
    x[2, :] = float('-inf'); x[2, 7] = 3.; x[2, 250] = 3.; x[2, 100] = 5.   # fewer finite values than k
    x[3] = torch.randn(300, device='cuda').round()   # many ties at the cut
    x[4] = -torch.arange(300.)
    vals, idx = ops.topk_dense(x, 100)
    rv, ri = oracle.topk(x.cpu().numpy(), 100)
    assert np.array_equal(idx.cpu().numpy(), ri)
    assert np.array_equal(vals.cpu().numpy(), rv)
    assert idx.dtype == torch.int64


@pytest.mark.parametrize('C', [9000, 16000])
def test_topk_wide_rows_fast_path_and_fallback(ops, oracle, C):
    """cols >= 4096: the row is held in registers (up to 12 288 / 16 384 columns: two kernels) and the candidates are
    the keys >= the k-th largest per-thread maximum (k <= 256), else a histogram's; rows whose candidates overflow LDS
    (long runs of equal values) fall back to the 4 x 8-bit radix select.  Exact ids either way."""
    g = torch.Generator(device='cuda').manual_seed(4)
    x = torch.randn(10, C, device='cuda', generator=g)
    x[1] = (x[1] * 2).round() / 2                         # ~1500 values per level: ties inside the candidate bin
    x[2, :] = 0.25                                        # one value everywhere: > 2048 candidates -> fallback
    x[3, :] = float('-inf'); x[3, ::97] = torch.randn(len(range(0, C, 97)), device='cuda', generator=g)   # 93 finite < k
    x[4] = torch.randn(C, device='cuda', generator=g) * 1e-30       # denormal-range magnitudes
    x[5, 4000:] = float('-inf')                           # the exclusion mask of a heavy user
    x[6] = -x[0]
    x[7] = torch.arange(C, device='cuda', dtype=torch.float32) % 50  # 180 copies of each level, k cuts through one
    x[8] = -torch.arange(C, device='cuda', dtype=torch.float32)      # sorted along the columns: the top k sit in a few
    x[9] = torch.arange(C, device='cuda', dtype=torch.float32)       # threads' registers (more candidates than 256)
    for k in (100, 5, 1, 2, 256, 300):
        vals, idx = ops.topk_dense(x, k)
        rv, ri = oracle.topk(x.cpu().numpy(), k)
        assert np.array_equal(idx.cpu().numpy(), ri), k
        assert np.array_equal(vals.cpu().numpy(), rv), k
    # an odd width (the ml10m catalogue): rows start at every offset from a 16-byte boundary (the shifted pieces)
    y = torch.randn(9, 10677, device='cuda', generator=g)
    vals, idx = ops.topk_dense(y, 100)
    rv, ri = oracle.topk(y.cpu().numpy(), 100)
    assert np.array_equal(idx.cpu().numpy(), ri) and np.array_equal(vals.cpu().numpy(), rv)


def test_rank_metrics_vs_reference_functions(ops):
    fx = load_golden('g5_metrics.npz')
    y = fx['y_true']
    R = y.shape[0]
    ptr, idx = csr_from_pairs(np.argwhere(y > 0), R)
    vals, ids = ops.topk_dense(dev(fx['logits']), 100)
    assert np.array_equal(ids.cpu().numpy(), fx['top100'])
    ks = [5, 10, 50, 100]
    m = ops.rank_metrics(ids.to(torch.int32), torch.arange(R, device='cuda'), dev(ptr), dev(idx), ks).cpu().numpy()
    for t, k in enumerate(ks):
        for j, name in enumerate(('precision', 'recall', 'ndcg')):
            np.testing.assert_allclose(m[:, t, j], fx[f'{name}@{k}'], rtol=1e-5, atol=1e-7, err_msg=f'{name}@{k}')


def test_full_size_properties_cfg3(ops):
    """BASELINE cfg3 shape (U=69878, I=10677, D=512, N=100, B=4096): size-independent properties.
    (1) linearity: with lr -> tiny the loss of step 2 equals the loss of step 1 recomputed by the un-fused
    operators; (2) every row moved (dense AdamW); (3) loss = log 2 at zero embeddings; (4) finite."""
    torch.manual_seed(1)
    U, I, D, B, N = 69878, 10677, 512, 4096, 100
    P = {'user_emb': torch.randn(U, D, device='cuda') * (0.1 / D) * 50, 'item_emb': torch.randn(I, D, device='cuda') * (0.1 / D) * 50,
         'item_bias': torch.randn(I, device='cuda') * 0.1}
    st = ops.BprMfFusedState(P['user_emb'], P['item_emb'], P['item_bias'], lr=3e-4, wd=4e-5, max_batch=B, max_cols=N + 1)
    u = torch.randint(0, U, (B,), device='cuda')
    i = torch.randint(0, I, (B, N + 1), device='cuda')
    logits = ops.mf_scores(P['user_emb'], P['item_emb'], P['item_bias'], None, None, u, i)
    loss_unfused, _ = ops.bpr_loss_grad(logits, need_grad=False)
    before_u = P['user_emb'][:64].clone()
    st.step(u, i)
    st.flush()
    assert abs(st.last_loss() - loss_unfused.item()) <= 1e-6 * loss_unfused.item()
    assert torch.isfinite(P['user_emb']).all() and torch.isfinite(P['item_emb']).all()
    touched = torch.zeros(U, dtype=torch.bool, device='cuda')
    touched[u] = True
    moved = (P['user_emb'][:64] != before_u).any(dim=1)
    # touched rows move by ~lr; untouched rows only decay by (1 - lr*wd)
    assert moved[touched[:64]].all()
    untouched = ~touched[:64]
    if untouched.any():
        ratio = (P['user_emb'][:64][untouched] / before_u[untouched])
        assert torch.allclose(ratio, torch.full_like(ratio, 1 - 3e-4 * 4e-5), rtol=1e-6)
    st.check_status()
    # zero embeddings & biases -> every x = 0 -> loss = log 2
    Z = {'user_emb': torch.zeros(1000, D, device='cuda'), 'item_emb': torch.zeros(I, D, device='cuda')}
    st2 = ops.BprMfFusedState(Z['user_emb'], Z['item_emb'], None, lr=1e-3, wd=0.0, max_batch=B, max_cols=N + 1)
    st2.step(torch.randint(0, 1000, (B,), device='cuda'), i)
    assert abs(st2.last_loss() - np.log(2.0)) < 1e-7  # softplus evaluated in fp32


def test_full_size_fused_step_equals_unfused_operator_chain(ops, oracle):
    """BASELINE configs[2] in full (ml10m-shaped synthetic interactions, D=512, N=100, B=4096): one device-sampled fused
    step -- sampler, item sort, forward, item pass, lazy user update -- against the un-fused HIP operators
    (hsk_mf_scores -> hsk_bpr_loss_grad -> hsk_mf_backward -> hsk_adamw_dense), which the small-shape tests pin to the
    reference's golden vectors.  Plus the sampler's invariants on the whole 4096 x 100 draw."""
    from hassaku_amd.data import synthetic
    from hassaku_amd.data.csr import UserItemCsr
    data = synthetic.generate_named('ml10m', seed=0)
    U, I, D, B, N = data.n_users, data.n_items, 512, 4096, 100
    csr = UserItemCsr.from_pairs(data.train[:, 0], data.train[:, 1], U, I)
    indptr, indices = csr.to_device('cuda')
    torch.manual_seed(64)
    P = {'user_emb': torch.empty((U, D), device='cuda').normal_(std=0.05), 'item_emb': torch.empty((I, D), device='cuda').normal_(std=0.05),
         'item_bias': torch.empty((I,), device='cuda').normal_(std=0.1)}
    Q = {k: v.clone() for k, v in P.items()}
    R0 = {k: v.cpu().numpy().copy() for k, v in P.items()}     # for the CPU oracle, below
    lr, wd = 3e-4, 4e-5
    st = ops.BprMfFusedState(P['user_emb'], P['item_emb'], P['item_bias'], lr=lr, wd=wd, max_batch=B, max_cols=N + 1, seed=64,
                             csr_indptr=indptr, csr_indices=indices,
                             coo_user=torch.from_numpy(data.train[:, 0].astype(np.int32)).cuda(),
                             coo_item=torch.from_numpy(data.train[:, 1].astype(np.int32)).cuda())
    order = torch.randperm(data.train.shape[0], device='cuda')
    st.step_sampled(order, 0, B, N)
    st.flush()
    st.check_status()
    u, i = st.last_batch(B, N + 1)
    sel = order[:B].cpu().numpy()
    assert np.array_equal(u.cpu().numpy(), data.train[sel, 0]) and np.array_equal(i[:, 0].cpu().numpy(), data.train[sel, 1])
    ptr_h, idx_h = csr.indptr, csr.indices
    assert oracle.count_bad_negatives(np.asarray(ptr_h), np.asarray(idx_h), I, u.cpu().numpy(), i[:, 1:].cpu().numpy()) == 0
    # the same step from the un-fused operators
    logits = ops.mf_scores(Q['user_emb'], Q['item_emb'], Q['item_bias'], None, None, u, i)
    loss, g = ops.bpr_loss_grad(logits)
    assert abs(st.last_loss() - loss.item()) <= 1e-6 * loss.item()
    assert float(g.sum(dim=1).abs().max()) < 1e-9            # BPR: the gradient wrt a row of logits sums to zero
    g_u, g_i, g_ib, _, _ = ops.mf_backward(Q['user_emb'], Q['item_emb'], u, i, g, True, False, False)
    for name, grad in (('user_emb', g_u), ('item_emb', g_i), ('item_bias', g_ib)):
        m, v = torch.zeros_like(Q[name]), torch.zeros_like(Q[name])
        ops.adamw_dense(Q[name], grad, m, v, lr, wd, 1)
        assert_adam_param_close(P[name].cpu().numpy(), Q[name].cpu().numpy(), name)
        assert max_norm_err(st.m[name].cpu().numpy(), m.cpu().numpy()) < 1e-5, name
        assert max_norm_err(st.v[name].cpu().numpy(), v.cpu().numpy()) < 1e-5, name
    # ... and from the CPU oracle (the restatement of the reference that the golden vectors pin): the full-size
    # 4096 x 101 x 512 batch the device sampled, one optimisation step -- loss to 1e-6, parameters by the Adam rule,
    # exp_avg / exp_avg_sq to 1e-5
    tr = oracle.MfOracleTrainer(R0['user_emb'], R0['item_emb'], R0['item_bias'], lr=lr, wd=wd)
    loss_ref = tr.step(u.cpu().numpy(), i.cpu().numpy())[0]
    assert abs(st.last_loss() - loss_ref) <= 1e-6 * loss_ref
    for name in ('user_emb', 'item_emb', 'item_bias'):
        assert_adam_param_close(P[name].cpu().numpy(), tr.P[name], 'oracle ' + name)
        assert max_norm_err(st.m[name].cpu().numpy(), tr.M[name]) < 1e-5, name
        assert max_norm_err(st.v[name].cpu().numpy(), tr.V[name]) < 1e-5, name


def test_last_batch_after_a_replayed_run_with_grouped_preparation(ops):
    """After a run of 64 replayed steps whose batches were prepared 8 at a time (k_prep_sample_group), last_batch /
    last_sort still show the batch of the final step -- the one an eager run of the same steps ends on."""
    rng = np.random.RandomState(12)
    n_users, n_items, D, B, N = 200, 500, 64, 128, 3
    pairs = np.argwhere(rng.rand(n_users, n_items) < 0.15)
    pairs = pairs[rng.permutation(len(pairs))]
    ptr, idx = csr_from_pairs(pairs, n_users)
    P = {'user_emb': (rng.randn(n_users, D) * 0.05).astype(np.float32),
         'item_emb': (rng.randn(n_items, D) * 0.05).astype(np.float32)}
    order = torch.from_numpy(np.random.RandomState(3).permutation(len(pairs))).cuda()
    assert order.numel() >= 64 * B
    out = []
    for chunked in (False, True):
        st, _ = _fused_state(ops, P, 1e-3, 0.0, B, N + 1, seed=5, csr_indptr=dev(ptr), csr_indices=dev(idx),
                             coo_user=dev(pairs[:, 0], torch.int32), coo_item=dev(pairs[:, 1], torch.int32))
        if chunked:
            st.steps_sampled(order, 0, 64, B, N)
            assert st.graph_replays() == 1
        else:
            for s in range(64):
                st.step_sampled(order, s * B, B, N)
        u, i = st.last_batch(B, N + 1)
        perm, offs = st.last_sort(B * (N + 1))
        out.append([x.cpu().numpy() for x in (u, i, perm, offs)])
        st.check_status()
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    assert np.array_equal(out[0][0], pairs[order[63 * B:64 * B].cpu().numpy(), 0])


def test_eval_cfg4_shape_eight_item_shards_vs_float64(ops):
    """BASELINE configs[3] at its own size on one device: D = 512, 131 072 items cut into the 8 range shards an 8-GPU
    node holds (physical shards, global ids, exclusion mask restricted to the range, top-k selected inside the GEMM),
    hsk_topk_merge -> per user the same top-100 as a float64 scoring of the whole catalogue (ids exact wherever the
    float64 scores are further apart than fp32 can resolve, values to 1e-5)."""
    torch.manual_seed(1)
    n_users, n_items, D, k, W = 256, 131072, 512, 100, 8
    U = torch.randn(n_users, D, device='cuda') * 0.05
    I = torch.randn(n_items, D, device='cuda') * 0.05
    Ib = torch.randn(n_items, device='cuda') * 0.1
    rng = np.random.RandomState(8)
    e_ptr, e_idx = _toy_csr(rng, n_users, n_items, 120.0 / n_items)
    u = torch.arange(n_users, device='cuda')
    parts_v, parts_i = [], []
    for r in range(W):
        lo, hi = n_items * r // W, n_items * (r + 1) // W
        v, i, sc = ops.mf_eval_topk(U, I[lo:hi].contiguous(), Ib[lo:hi].contiguous(), None, None, u, k, dev(e_ptr), dev(e_idx),
                                    item_begin=lo, item_count=hi - lo, item_shard=True, n_items_global=n_items,
                                    want_scores=(r % 2 == 1))   # even shards: selection inside the GEMM; odd: materialised
        assert (sc is None) == (r % 2 == 0)
        parts_v.append(v)
        parts_i.append(i)
    mv, mi = ops.topk_merge(torch.stack(parts_v).contiguous(), torch.stack(parts_i).contiguous())
    ref = U.double() @ I.double().T + Ib.double()[None, :]
    ptr, idx = e_ptr, e_idx
    for r in range(n_users):
        ref[r, torch.from_numpy(idx[ptr[r]:ptr[r + 1]].astype(np.int64)).cuda()] = float('-inf')
    rv, ri = torch.topk(ref, k + 1, dim=1)
    assert torch.allclose(mv.double(), rv[:, :k], rtol=1e-5, atol=1e-6)
    gap = (rv[:, :-1] - rv[:, 1:]) > 1e-5            # ranks whose neighbours are clearly apart
    clear = gap & torch.cat([torch.ones_like(gap[:, :1]), gap[:, :-1]], dim=1)
    assert clear.float().mean() > 0.9
    assert torch.equal(mi.long()[clear], ri[:, :k][clear])


def test_hyper_parameters_are_frozen_and_set_hyper_re_prepares(ops):
    """lr / wd / betas / eps live in a device table of per-step Adam scalars (lazy replay, replayed graphs) computed when
    the workspace is prepared: a step that finds st.lr changed FAILS (it would otherwise mix two schedules, or replay a
    graph with the old value frozen into it); set_hyper() -- flush under the old values, new values, workspace prepared
    again, captured graphs dropped -- is the way, and a run issued as replayed graphs then equals the same steps issued
    one by one, bit for bit, across three LR changes."""
    n_users, n_items, D, B, N = 300, 900, 64, 128, 6
    rng = np.random.RandomState(4)
    pairs = np.argwhere(rng.rand(n_users, n_items) < 0.15)
    pairs = pairs[rng.permutation(len(pairs))]
    ptr, idx = csr_from_pairs(pairs, n_users)
    P = {'user_emb': (rng.randn(n_users, D) * 0.05).astype(np.float32),
         'item_emb': (rng.randn(n_items, D) * 0.05).astype(np.float32),
         'item_bias': (rng.randn(n_items) * 0.1).astype(np.float32)}
    order = torch.from_numpy(np.concatenate([np.random.RandomState(r).permutation(len(pairs)) for r in range(2)])).cuda()
    res = []
    for chunked in (False, True):
        st, t = _fused_state(ops, P, 1e-3, 1e-4, B, N + 1, seed=5, csr_indptr=dev(ptr), csr_indices=dev(idx),
                             coo_user=dev(pairs[:, 0], torch.int32), coo_item=dev(pairs[:, 1], torch.int32))
        st.st.nnz = order.numel()
        for run, lr in enumerate((1e-3, 5e-2, 1e-3)):          # back to the first value: no stale graph may survive
            if run:
                st.set_hyper(lr=lr)
            if chunked:
                st.steps_sampled(order, run * 64 * B, 64, B, N)
            else:
                for s in range(64):
                    st.step_sampled(order, (run * 64 + s) * B, B, N)
        st.flush()
        st.check_status()
        assert st.graph_replays() == (3 if chunked else 0) and st.step_count == 192
        res.append(({k: v.cpu().numpy().copy() for k, v in t.items()}, st.pop_loss_sum()))
    assert res[0][1] == res[1][1]
    for k in res[0][0]:
        assert np.array_equal(res[0][0][k], res[1][0][k]), k
    # the raw field changed behind the library's back: refused, not obeyed
    st.st.lr = 0.5
    with pytest.raises(RuntimeError, match='init_workspace'):
        st.step_sampled(order, 0, B, N)
    st.st.lr = 1e-3
    st.step_sampled(order, 0, B, N)


def test_score_all_fast_path_is_not_keyed_on_the_address():
    """_score_all remembers 'i_idxs is arange(n_items)' per tensor OBJECT: a permutation that the caching allocator
    places at the freed arange's address must take the general path (scores in the order of the given ids)."""
    from hassaku_amd.algorithms.sgd_alg import SGDMatrixFactorization
    torch.manual_seed(3)
    m = SGDMatrixFactorization(50, 4096, 32, False, True, False).to('cuda')
    u = torch.arange(8, device='cuda')
    ar = torch.arange(4096, device='cuda')
    full = m.combine_user_item_representations(m.get_user_representations(u), m.get_item_representations(ar))
    addr = ar.data_ptr()
    del ar
    perm = torch.randperm(4096, device='cuda')
    same_block = perm.data_ptr() == addr          # what the caching allocator usually does
    out = m.combine_user_item_representations(m.get_user_representations(u), m.get_item_representations(perm))
    assert torch.allclose(out, full[:, perm], rtol=1e-5, atol=1e-7), same_block
    assert not torch.equal(out, full)


def test_bench_eval_pass_vs_oracle(ops, oracle):
    """The evaluation pass bench.py TIMES (BASELINE configs[3] shape: 16 384 users x 131 072 items, D = 512, one
    16 384-user chunk, top-100 selected inside the score GEMM, 120 excluded positives per user), value-checked against
    the ORACLE (oracle.eval_scores + oracle.topk + oracle.rank_metrics, eval/eval.py:54-75,237-253 of the reference)
    on a sample of its users -- and the same users through the 8 physical item shards + hsk_topk_merge."""
    import bench
    U, I, D, _ = bench.EVAL_SHAPES['lfm2b']
    user_emb, item_emb, item_bias, ds = bench.eval_problem('lfm2b', torch.device('cuda'))
    arr = ds.device_arrays('cuda')
    ks = [100, 50, 10, 5]
    u_all = torch.arange(U, device='cuda')
    vals, ids, sc = ops.mf_eval_topk(user_emb, item_emb, item_bias, None, None, u_all, 100, arr['excl_indptr'],
                                     arr['excl_indices'])
    assert sc is None                                    # the fused path: no score matrix
    met = ops.rank_metrics(ids, u_all, arr['label_indptr'], arr['label_indices'], ks).cpu().numpy()
    sample = np.sort(np.random.RandomState(5).choice(U, size=96, replace=False))
    sample[0], sample[-1] = 0, U - 1
    Uh, Ih, Ibh = (t.cpu().numpy() for t in (user_emb, item_emb, item_bias))
    eptr, eidx = ds.exclude_csr.indptr, ds.exclude_csr.indices
    ref = oracle.eval_scores(Uh, Ih, Ibh, None, None, sample, eptr, eidx)
    rv, ri = oracle.topk(ref, 101)
    scale = np.abs(rv[:, :100]).max()

    def check(v, i, what):
        v, i = v.cpu().numpy(), i.cpu().numpy().astype(np.int64)
        assert np.abs(v - rv[:, :100]).max() <= 1e-5 * scale, what
        gap = (rv[:, :-1] - rv[:, 1:]) > 2e-5 * scale    # ranks whose neighbours fp32 sums can tell apart
        clear = gap[:, :100] & np.concatenate([np.ones((len(sample), 1), bool), gap[:, :99]], axis=1)
        assert clear.mean() > 0.9, what
        assert np.array_equal(i[clear], ri[:, :100][clear]), what
        # never an excluded item, never a duplicate
        for r, uu in enumerate(sample):
            assert not np.isin(i[r], eidx[eptr[uu]:eptr[uu + 1]]).any() and len(np.unique(i[r])) == 100, what

    sel = torch.from_numpy(sample).cuda()
    check(vals[sel], ids[sel], 'fused pass')
    ref_met = oracle.rank_metrics(ri[:, :100], sample, ds.label_csr.indptr, ds.label_csr.indices, ks)
    unambiguous = np.array([np.array_equal(ids[u].cpu().numpy(), ri[r, :100]) for r, u in enumerate(sample)])
    assert unambiguous.mean() > 0.5
    np.testing.assert_allclose(met[sample][unambiguous], ref_met[unambiguous], rtol=1e-6, atol=1e-7)
    # the 8 physical item shards of an 8-GPU node (global ids, mask restricted to the range) + the merge
    W = 8
    pv, pi = [], []
    for r in range(W):
        lo, hi = I * r // W, I * (r + 1) // W
        v, i, _ = ops.mf_eval_topk(user_emb, item_emb[lo:hi].contiguous(), item_bias[lo:hi].contiguous(), None, None, sel, 100,
                                   arr['excl_indptr'], arr['excl_indices'], item_begin=lo, item_count=hi - lo,
                                   item_shard=True, n_items_global=I)
        pv.append(v)
        pi.append(i)
    mv, mi = ops.topk_merge(torch.stack(pv).contiguous(), torch.stack(pi).contiguous())
    check(mv, mi, '8-shard merge')
