"""CPU checks of the variational link heads: the float64 restatement tests/var_head_ref.py against the reference's own fixture
(g4_vae.npz) and against torch autograd, every planted defect against the bound the device test uses, the builders' properties, the
model / trainer / command-line surface without a GPU, and the refusals of the two entries that return before a launch."""
import ctypes
import math

import numpy as np
import pytest
import torch

import dense_ref as DR
import var_head_ref as VR
from conftest import load_golden
from var_head_ref import F64

U24 = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ restatement
def test_restatement_reproduces_the_reference_fixture():
    """sample_*, s_kl, t_kl and, with up_*, kl_weight, every grad_* of g4_vae.npz.  Bound: the fixture is float32 arithmetic; an
    entry is a float32 sum of at most L = 2H + N + 8 terms (a head's H products and bias, then N rows of a weight gradient or 2H
    columns of an input gradient), so it lies within L 2^-24 of the exact value on the entry's scale."""
    z = load_golden('g4_vae')
    c = VR.fixture_case(z)
    r = VR.exact(c)
    want = VR.fixture_expected(z)
    bound = (2 * c['H'] + c['N'] + 8) * U24
    for k in ('Z', 'dST', 'dWp_s', 'dWp_t', 'dbp_s', 'dbp_t'):
        q = DR.ratio(want[k], r[k], r['S'][k])
        assert q <= bound, (k, q, bound)
    q = DR.ratio(want['kl_loss'], c['klcoef'] * r['kl'], abs(c['klcoef']) * r['S']['kl'])
    assert q <= bound, ('kl', q, bound)


def test_restatement_equals_torch_autograd():
    """Linear + exp + the KL expression of trainer.py:146-147 in float64 under autograd."""
    c = VR.case(32, 70, seed=3)
    r = VR.exact(c)
    H = c['H']
    st = c['ST'][:, :2 * H].to(F64).requires_grad_(True)
    Wp = [w.to(F64).requires_grad_(True) for w in c['Wp']]
    bp = [b.to(F64).requires_grad_(True) for b in c['bp']]
    zs, kls = [], []
    for h in (0, 1):
        P = torch.nn.functional.linear(st[:, h * H:(h + 1) * H], Wp[h], bp[h])
        mu, ls = P[:, :H], P[:, H:]
        zs.append(mu + torch.exp(ls) * c['eps'][:, h * H:(h + 1) * H].to(F64))
        kls.append(torch.sum(1 + 2 * ls - mu ** 2 - torch.exp(ls) ** 2))
    Z = torch.cat(zs, 1)
    gk = [float(np.float32(g)) for g in c['gkl']]
    ((Z * c['gZ'][:, :2 * H].to(F64)).sum() + gk[0] * kls[0] + gk[1] * kls[1]).backward()
    got = {'Z': Z.detach(), 'kl': torch.stack(kls).detach(), 'dST': st.grad, 'dWp_s': Wp[0].grad, 'dWp_t': Wp[1].grad,
           'dbp_s': bp[0].grad, 'dbp_t': bp[1].grad}
    for k, q in VR.ratios(got, r).items():
        assert q <= 64 * 2.0 ** -53, (k, q)
    # and, on its own [mu | ls], tests/losses_ref.reparam (the restatement the reparameterisation kernels are held to), per half
    import losses_ref as LR
    for h in (0, 1):
        P = r['ML'][:, 2 * H * h:2 * H * (h + 1)]
        cols = slice(h * H, (h + 1) * H)
        q = LR.reparam(P[:, :H], P[:, H:], c['eps'][:, cols], gz=c['gZ'][:, cols], gkl=float(np.float32(c['gkl'][h])))
        assert torch.allclose(q['z'], r['Z'][:, cols], rtol=0, atol=1e-13) and abs(float(q['kl'] - r['kl'][h])) <= 1e-9
        dP = torch.cat([q['dmu'], q['dls']], 1)
        assert torch.allclose(dP @ c['Wp'][h].to(F64), r['dST'][:, cols], rtol=0, atol=1e-11)


@pytest.mark.parametrize('H', VR.WIDTHS)
def test_stand_in_is_close_and_bounds_are_finite(H):
    c = VR.case(H, 129, seed=1)
    r64, rk = VR.exact(c), VR.stand_in(c)
    tau = VR.taus(r64, rk)
    assert set(tau) == {'Z', 'ML', 'kl', 'dST', 'dWp_s', 'dWp_t', 'dbp_s', 'dbp_t'}
    for k, t in tau.items():
        assert 8 * DR.FLOOR['x3'] <= t < 1e-3, (k, t)


def _defect_cases():
    H = 64
    g = VR.nwg('var_head_bwd', H, VR.cap_rows('var_head_bwd', H) + 1)
    return [
        (('seed_t',), dict(eps='gen'), 129, ('Z',)),
        (('swap_rows',), {}, 129, ('Z', 'ML', 'kl', 'dST')),
        (('no_2ls',), {}, 129, ('kl',)),
        (('dls_no_eps',), {}, 129, ('dST', 'dWp_s', 'dbp_t')),
        (('sample0_noise',), dict(sample=0), 129, ('Z',)),
        (('drop_last_tile_kl',), {}, 70, ('kl',)),          # the fixture's size: 6 rows of 70 (one row of 129 is 3 tau)
        (('dwp_tile_lost', g), {}, VR.cap_rows('var_head_bwd', H) + TILE_ROWS, ('dWp_s', 'dWp_t', 'dbp_s', 'dbp_t')),
    ]


TILE_ROWS = VR.TILE


@pytest.mark.parametrize('k', range(7))
def test_planted_defects_lie_ten_times_outside_the_device_bound(k):
    mutate, opts, N, outputs = _defect_cases()[k]
    c = VR.case(64, N, seed=2)
    r64 = VR.exact(c, **opts)
    tau = VR.taus(r64, VR.stand_in(c, **opts))
    bad = VR.ratios(VR.stand_in(c, mutate=mutate, **opts), r64)
    for o in outputs:
        assert bad[o] >= 10 * tau[o], (mutate, o, bad[o], tau[o])


def test_builders():
    for H in VR.WIDTHS:
        for wide in (False, True):
            c = VR.case(H, 130, seed=4, wide=wide)
            assert c['ST'].shape == (130, 2 * H + (8 if wide else 0)) and c['ST'].shape[1] % 4 == 0
            assert bool(torch.isnan(c['ST'][:, 2 * H:]).all()) and bool(torch.isfinite(c['ST'][:, :2 * H]).all())
            assert bool(torch.isnan(c['gZ'][:, 2 * H:]).all()) and bool(torch.isnan(c['eps'][:, 2 * H:]).all())
            r = VR.exact(c)
            for h in (0, 1):
                ls = r['ML'][:, h * 2 * H + H:(h + 1) * 2 * H]
                assert float(ls.min()) < VR.LS_LO + 0.1 and float(ls.max()) > VR.LS_HI - 0.1
                assert float(ls.min()) > VR.LS_LO - 0.1 and float(ls.max()) < VR.LS_HI + 0.1
    a, b = VR.case(32, 70, seed=5), VR.case(32, 70, seed=5)
    assert torch.equal(a['ST'], b['ST']) and torch.equal(a['Wp'][1], b['Wp'][1])
    # the generated noise: per half its own seed, element r * H + c
    e = VR.noise(32, 5, 9)
    assert e.shape == (5, 64) and not torch.equal(e[:, :32], e[:, 32:])
    import losses_ref as LR
    assert np.array_equal(e[:, 32:].reshape(-1).numpy(), LR.gauss_from_counter(10, 160))


def test_geometry_restated():
    assert VR.fwd_smem(64) == 54272 and VR.per_cu('var_head_fwd', 64) == 3 and VR.per_cu('var_head_fwd', 32) == 4
    assert VR.bwd_smem(64) == 77824 and VR.bwd_smem(32) == 18432 + 10240 + 4096
    assert VR.cap_rows('var_head_bwd', 64) == 8192 and VR.cap_rows('var_head_fwd', 64) == 24576
    for k in VR.GEOMETRY:
        for H in VR.WIDTHS:
            n = VR.large_rows(k, H)
            assert n <= 400000 and n % VR.TILE == 19
            assert VR.nwg(k, H, n) == 128 * VR.per_cu(k, H) and VR.nwg(k, H, 65) == 2 and VR.nwg(k, H, 0) == 1


# ------------------------------------------------------------------------------------------------ library surface without a GPU
def _entry(name):
    from deepgate import _hip
    return getattr(_hip.load(), name)


def test_workspace_size_entry():
    f = _entry('mgv_var_head_x3_ws_floats')
    for H in VR.WIDTHS:
        for N in (0, 1, 64, 65, 70, VR.cap_rows('var_head_bwd', H) + 1, VR.large_rows('var_head_fwd', H)):
            assert f(H, N, 0) == VR.ws_floats(H, N, False) and f(H, N, 1) == VR.ws_floats(H, N, True)
    assert f(16, 64, 0) == 0 and f(128, 64, 1) == 0 and f(64, -1, 0) == 0


def _fwd_args(H=64, N=70, **over):
    p = lambda k: ctypes.c_void_p(4096 * k)       # noqa: E731  (distinct, aligned, never read: every call returns before a launch)
    a = dict(H=H, N=N, ST=p(1), ldst=2 * H, wpack_s=p(2), wpack_t=p(3), b_s=p(4), b_t=p(5), eps=p(6), ldeps=2 * H, seed=1, sample=1,
             Z=p(7), ldz=2 * H, ML=p(8), ldml=4 * H, klsum=p(9), workspace=p(10), workspace_floats=1 << 30, stream=None)
    a.update(over)
    return list(a.values())


def _bwd_args(H=64, N=70, **over):
    p = lambda k: ctypes.c_void_p(4096 * k)       # noqa: E731
    a = dict(H=H, N=N, ST=p(1), ldst=2 * H, wpack_s=p(2), wpack_t=p(3), wtpack_s=p(4), wtpack_t=p(5), b_s=p(6), b_t=p(7), eps=p(8),
             ldeps=2 * H, seed=1, sample=1, gZ=p(9), ldg=2 * H, gkl=p(10), dST=p(11), lddst=2 * H, dWp_s=p(12), dWp_t=p(13), dbp_s=p(14),
             dbp_t=p(15), workspace=p(16), workspace_floats=1 << 30, stream=None)
    a.update(over)
    return list(a.values())


def test_refusals_before_a_launch():
    fwd, bwd = _entry('mgv_var_head_fwd_x3'), _entry('mgv_var_head_bwd_x3')
    EINVAL, EUNSUPPORTED = -1, -2
    for H in (0, 16, 48, 128):
        assert fwd(*_fwd_args(H=H)) == EUNSUPPORTED and bwd(*_bwd_args(H=H)) == EUNSUPPORTED
        assert fwd(*_fwd_args(H=H, ST=None)) == EUNSUPPORTED            # the width comes first
    for H in VR.WIDTHS:
        assert fwd(*_fwd_args(H=H, N=0)) == 0 and bwd(*_bwd_args(H=H, N=0)) == 0      # nothing to do, nothing launched
        for k in ('ST', 'wpack_s', 'wpack_t', 'b_s', 'b_t', 'Z', 'klsum', 'workspace'):
            assert fwd(*_fwd_args(H=H, **{k: None})) == EINVAL, k
        for k in ('ST', 'wpack_s', 'wpack_t', 'wtpack_s', 'wtpack_t', 'b_s', 'b_t', 'dST', 'dWp_s', 'dWp_t', 'dbp_s', 'dbp_t', 'workspace'):
            assert bwd(*_bwd_args(H=H, **{k: None})) == EINVAL, k
        assert fwd(*_fwd_args(H=H, N=-1)) == EINVAL and bwd(*_bwd_args(H=H, N=-1)) == EINVAL
        for k in ('ldst', 'ldz', 'ldeps', 'ldml'):
            w = 4 * H if k == 'ldml' else 2 * H
            assert fwd(*_fwd_args(H=H, **{k: w - 4})) == EINVAL and fwd(*_fwd_args(H=H, **{k: w + 2})) == EINVAL, k
        for k in ('ldst', 'lddst', 'ldeps', 'ldg'):
            assert bwd(*_bwd_args(H=H, **{k: 2 * H - 4})) == EINVAL and bwd(*_bwd_args(H=H, **{k: 2 * H + 2})) == EINVAL, k
        assert fwd(*_fwd_args(H=H, sample=2)) == EINVAL and bwd(*_bwd_args(H=H, sample=-1)) == EINVAL
        # a NULL eps / ML / gZ / gkl is allowed, and then their strides are not looked at: the call goes on to the workspace check
        assert fwd(*_fwd_args(H=H, workspace_floats=VR.ws_floats(H, 70, False) - 1)) == EINVAL
        assert fwd(*_fwd_args(H=H, eps=None, ldeps=0, ML=None, ldml=0, workspace_floats=VR.ws_floats(H, 70, False) - 1)) == EINVAL
        assert fwd(*_fwd_args(H=H, workspace=ctypes.c_void_p(4100))) == EINVAL       # doubles live there
        assert bwd(*_bwd_args(H=H, workspace_floats=VR.ws_floats(H, 70, True) - 1)) == EINVAL
        assert bwd(*_bwd_args(H=H, gZ=None, ldg=0, gkl=None, eps=None, ldeps=0, workspace_floats=VR.ws_floats(H, 70, True) - 1)) == EINVAL


# ------------------------------------------------------------------------------------------------ model surface without a GPU
def _model(variational, H=32, seed=11, baseline=False):
    import deepgate
    torch.manual_seed(seed)
    if baseline:
        enc = deepgate.digae_layer.DirectedGCNConvEncoder(in_channels=6, hidden_channels=H, out_channels=H, alpha=1.0, beta=0.0,
                                                          self_loops=True, adaptive=False)
    else:
        enc = deepgate.digae_layer.DirectMultiGCNEncoder(dim_hidden=H, dim_feature=6, s_rounds=1, t_rounds=1, layernorm=True)
    return deepgate.dg_ae_model_aig.Model(struct_encoder=enc, dim_hidden=H, **({'variational': True} if variational else {}))


HEADS = ['fc_s_mu', 'fc_s_logstd', 'fc_t_mu', 'fc_t_logstd']


@pytest.mark.parametrize('baseline', [False, True])
def test_variational_model_registers_the_heads_last(baseline):
    plain, var = _model(False, baseline=baseline), _model(True, baseline=baseline)
    kp, kv = list(plain.state_dict()), list(var.state_dict())
    assert kv[:len(kp)] == kp and kv[len(kp):] == [h + s for h in HEADS for s in ('.weight', '.bias')]
    assert plain.variational is False and var.variational is True
    for k in kp:
        assert torch.equal(plain.state_dict()[k], var.state_dict()[k]), k
    assert all(getattr(var, h).weight.shape == (32, 32) for h in HEADS) and not any(hasattr(plain, h) for h in HEADS)
    with pytest.raises(ValueError):
        plain.latent(torch.zeros(2, 32))
    with pytest.raises(ValueError):
        var.kl_loss()                      # no recon_loss yet


def test_dg_ae_checkpoint_loads_into_a_variational_model(tmp_path, capsys):
    plain, var = _model(False, seed=3), _model(True, seed=4)
    path = str(tmp_path / 'ae.pth')
    torch.save({'epoch': 0, 'state_dict': plain.state_dict()}, path)
    before = {h: getattr(var, h).weight.clone() for h in HEADS}
    var.load(path)
    out = capsys.readouterr().out
    assert out.count('No param') == 8 and all('No param %s.weight.' % h in out for h in HEADS)
    for k, v in plain.state_dict().items():
        assert torch.equal(var.state_dict()[k], v), k
    assert all(torch.equal(getattr(var, h).weight, before[h]) for h in HEADS)
    # and the other way: a variational checkpoint into a variational model, strict
    var2 = _model(True, seed=5)
    var2.load_state_dict(var.state_dict(), strict=True)


def test_train_main_reaches_the_trainer_with_a_variational_model(monkeypatch, tmp_path):
    import deepgate
    import train
    seen = {}

    class Stop(Exception):
        pass

    def fake_trainer(args, model, **kw):
        seen.update(args=args, model=model)
        raise Stop

    monkeypatch.setattr(deepgate, 'Trainer', fake_trainer)
    argv = ['--exp_id', 'v', '--type', 'aig', '--synthetic', '2', '--synthetic_nodes', '64', '--synthetic_levels', '4', '--save_dir', str(tmp_path),
            '--dim_hidden', '32']
    for name in ('DG_AE', 'AE'):
        with pytest.raises(Stop):
            train.main(argv + ['--model', name, '--variational', '--kl_weight', '0.25'])
        assert seen['model'].variational and all(hasattr(seen['model'], h) for h in HEADS)
        assert seen['args'].variational is True and seen['args'].kl_weight == 0.25
    with pytest.raises(Stop):
        train.main(argv + ['--model', 'DG_AE'])
    assert not seen['model'].variational and seen['args'].kl_weight == 0.0 and not any(hasattr(seen['model'], h) for h in HEADS)
    with pytest.raises(SystemExit, match='DG_VAE') as e:
        train.main(argv + ['--model', 'DG_VAE', '--variational'])
    assert '--model DG_AE --variational' in str(e.value)


def test_weighted_loss_adds_the_kl_term_only_under_a_positive_weight():
    from deepgate.trainer import Trainer
    t = Trainer.__new__(Trainer)
    t.rc_prob_func_weight = [1.0, 4.0, 2.0]
    ls = {'recon_loss': torch.tensor(0.5), 'prob_loss': torch.tensor(0.25), 'func_loss': torch.tensor(0.125), 'kl_loss': torch.tensor(8.0)}
    base = 0.5 + 1.0 + 0.25
    t.kl_weight = 0.0
    assert float(t.weighted_loss(ls)) == base
    t.kl_weight = 0.5
    assert float(t.weighted_loss(ls)) == base + 4.0
    assert float(t.weighted_loss({k: v for k, v in ls.items() if k != 'kl_loss'})) == base
    t.kl_weight = -1.0
    assert float(t.weighted_loss(ls)) == base


def test_trainer_reads_kl_weight_from_its_arguments(tmp_path):
    from types import SimpleNamespace

    from deepgate.trainer import Trainer
    for args, want in ((SimpleNamespace(model='DG_AE'), 0.0), (SimpleNamespace(model='DG_AE', kl_weight=0.5), 0.5)):
        t = Trainer(args, _model(True), save_dir=str(tmp_path), device='cpu', distributed=False)
        assert t.kl_weight == want and math.isfinite(t.kl_weight)


def test_metrics_carry_an_eighth_slot_only_with_a_kl_loss():
    from deepgate.trainer import Trainer
    t = Trainer.__new__(Trainer)
    ls = {'recon_loss': torch.tensor(0.5), 'prob_loss': torch.tensor(0.25), 'func_loss': torch.tensor(0.125),
          'confusion': torch.tensor([1, 2, 3, 4])}
    assert t.enqueue_metrics(ls) is None
    assert t.flush_metrics() == [0.5, 0.25, 0.125, 1.0, 2.0, 3.0, 4.0]
    t.enqueue_metrics(dict(ls, kl_loss=torch.tensor(2.0)))
    assert t.flush_metrics() == [0.5, 0.25, 0.125, 1.0, 2.0, 3.0, 4.0, 2.0]
