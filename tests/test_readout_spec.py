"""Pin the float64 restatements of the readout entries (tests/readout_ref.py) where there is no GPU: against torch autograd in float64
(batch_norm in training and eval mode -> relu -> the restated mask -> linear -> clamp; l1_loss), against oracle/ref_cpu.readout_prob
with the restated masks, and against the reference project's fixtures within their float32 arithmetic; assert the properties of the
builders that tests/test_hip_readout_entries.py relies on (band, cap edges, the partial U = 4 group, the two grids of B3); and show
that every planted defect lands at least ten times outside the bound the device test uses for that output.  CPU only.

MEASURED (this file, 2026-10-18): the float64 pins agree to 9.4e-13 of scale at worst (asserted: 1e-9)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import readout_ref as RR
from conftest import load_golden
from oracle import ref_cpu as R

F64, F32 = torch.float64, torch.float32
PIN = 1e-9
C, D = RR.CF, RR.D


def _pin(got, ref, S, what):
    r = RR.ratio(got, ref.detach(), S)
    print('PIN %s %.3g' % (what, r))
    assert r <= PIN, (what, r)


# ------------------------------------------------------------------------------------------------ torch autograd in float64
@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('Cw,N', [(4, 257), (8, 65), (16, 63), (32, 129), (64, 33)])
def test_bn_relu_drop_block_equals_torch_autograd(Cw, N, training):
    c = RR.layer_case(Cw, N)
    Y = c['Y'].to(F64).requires_grad_(True)
    gamma, beta = c['gamma'].to(F64).requires_grad_(True), c['beta'].to(F64).requires_grad_(True)
    if training:
        bn = F.batch_norm(Y, None, None, gamma, beta, training=True, eps=RR.BN_EPS)
        mean = Y.detach().mean(0)
        invstd = 1.0 / torch.sqrt(Y.detach().var(0, unbiased=False) + RR.BN_EPS)
    else:
        rm, rv = c['mean'].to(F64) + 0.3, (1.0 / c['invstd'].to(F64) ** 2) * 1.7
        bn = F.batch_norm(Y, rm, rv, gamma, beta, training=False, eps=RR.BN_EPS)
        mean, invstd = rm, 1.0 / torch.sqrt(rv + RR.BN_EPS)
    f = R.drop_factors(c['seed'], N, Cw, c['p'])
    A = F.relu(bn) * f
    dA = c['dA'].to(F64)
    dY, dg, db = torch.autograd.grad(A, (Y, gamma, beta), dA)
    a = (c['Y'], mean, invstd, c['gamma'], c['beta'], c['p'], c['seed'])
    fw = RR.bn_act_fwd(*a)
    _pin(fw['A'], A, fw['S']['A'], 'A')
    a0 = torch.arange(2 * Cw, dtype=F64) - 3.0
    bw = RR.bn_act_bwd(*a, c['dA'], sums0=a0)
    _pin(bw['sums'][:Cw] - a0[:Cw], db, bw['S']['sums'][:Cw], 'dbeta')
    _pin(bw['sums'][Cw:] - a0[Cw:], dg, bw['S']['sums'][Cw:], 'dgamma')
    ap = RR.bn_bwd_apply(c['Y'], mean, invstd, c['gamma'], bw['dZ'], bw['sums'] - a0, int(training))
    _pin(ap['dY'], dY, ap['S']['dY'], 'dY')
    assert bool((fw['A'][:, RR.DEAD_COL] == 0).all()) and bool((bw['dZ'][:, RR.DEAD_COL] == 0).all())
    if N > 1:
        assert bool((bw['dZ'][N // 2] == 0).all())


@pytest.mark.parametrize('clamp01', [0, 1])
@pytest.mark.parametrize('Cw,N', [(4, 257), (8, 65), (16, 63), (32, 129), (64, 33)])
def test_head_equals_torch_autograd(Cw, N, clamp01):
    c = RR.head_case(Cw, N)
    A, w, b = (c[k].to(F64).requires_grad_(True) for k in ('A', 'w', 'b'))
    h = F.linear(A, w[None], b)[:, 0]
    prob = torch.clamp(h, 0, 1) if clamp01 else h
    dA, dw, db = torch.autograd.grad(prob, (A, w, b), c['dprob'].to(F64))
    fw = RR.head_fwd(c['A'], c['w'], c['b'], clamp01)
    _pin(fw['prob'], prob, fw['S']['prob'], 'prob')
    dw0, db0 = torch.arange(Cw, dtype=F64), torch.tensor([-2.5], dtype=F64)
    bw = RR.head_bwd(c['A'], c['w'], c['b'], clamp01, c['dprob'], dw0, db0)
    _pin(bw['dA'], dA, bw['S']['dA'], 'dA')
    _pin(bw['dw'] - dw0, dw, bw['S']['dw'], 'dw')
    _pin(bw['db'] - db0, db, bw['S']['db'], 'db')
    if clamp01:
        inside = float(bw['inside'].double().mean())
        assert N < 60 or 0.1 < inside < 0.95, inside           # rows on both sides of the clamp


@pytest.mark.parametrize('gscale', [1.0, -0.37])
def test_l1_equals_torch_autograd(gscale):
    c = RR.l1_case(257)
    x = c['x'].to(F64).requires_grad_(True)
    loss = F.l1_loss(x, c['t'].to(F64))
    dx, = torch.autograd.grad(loss * float(np.float32(gscale)), x)
    fw = RR.l1_fwd(c['x'], c['t'], 5.0)
    assert abs(float(fw['sum'][0]) - 5.0 - 257 * float(loss.detach())) <= PIN * float(fw['S']['sum'][0])
    bw = RR.l1_bwd(c['x'], c['t'], gscale)
    assert float((bw['dx'] - dx).abs().max()) <= PIN * abs(gscale) / 257
    assert int(c['tie'].sum()) >= 64 and bool((bw['dx'][c['tie']] == 0).all()) and bool((bw['dx'][~c['tie']] != 0).all())


def test_colstats_reads_C_columns_of_ld():
    c = RR.layer_case(8, 65)
    for ld in (8, 12, 16, 72):
        Y = torch.full((65, ld), float('nan'))
        Y[:, :8] = c['Y']
        a0 = torch.arange(16, dtype=F64)
        r = RR.colstats(Y, ld, 8, a0)
        y = c['Y'].to(F64)
        assert torch.allclose(r['sums'] - a0, torch.cat([y.sum(0), (y * y).sum(0)]), rtol=1e-13, atol=0)
        assert float(r['sums'][8 + RR.CONST_COL] - a0[8 + RR.CONST_COL]) == 65 * 9.0


# ------------------------------------------------------------------------------------------------ the fused stages
def _oracle_params(c, grad=True):
    names = {'fc.0.weight': 'W1', 'fc.0.bias': 'b1', 'fc.1.weight': 'g1', 'fc.1.bias': 'be1', 'fc.4.weight': 'W2', 'fc.4.bias': 'b2',
             'fc.5.weight': 'g2', 'fc.5.bias': 'be2', 'fc.8.bias': 'b3'}
    p = {'readout_prob.' + k: c[v].to(F64).clone().requires_grad_(grad) for k, v in names.items()}
    p['readout_prob.fc.8.weight'] = c['w3'].to(F64)[None].clone().requires_grad_(grad)
    bn = {'readout_prob.fc.%d.running_%s' % (b, n): c['r%s%d' % (n[0], k)].to(F64).clone() for b, k in ((1, 1), (5, 2)) for n in ('mean', 'var')}
    return p, bn


@functools.lru_cache(maxsize=None)
def _fused(N, opt='A'):
    kw = {'A': {}, 'B': dict(clamp01=0, p=(0.0, 0.0), seeds=(77, 78)), 'D': dict(momentum=0.3, keep=0.6, eps=1e-3)}[opt]
    c = RR.fused_case(N, **kw)
    return c, RR.fused_fwd_stages(c)


@pytest.mark.parametrize('N,opt', [(2, 'A'), (65, 'A'), (129, 'A'), (129, 'B'), (4099, 'A')])
def test_fused_stages_equal_the_oracle_readout(N, opt):
    """Forward, running buffers and every gradient of oracle.ref_cpu.readout_prob (torch autograd, float64, the restated masks)."""
    c, r = _fused(N, opt)
    p, bn = _oracle_params(c)
    x = c['hf'].to(F64).requires_grad_(True)
    drop = [R.drop_factors(c['seed1'], N, C, c['p1']), R.drop_factors(c['seed2'], N, C, c['p2'])]
    prob = R.readout_prob(p, x, True, bn, momentum=c['momentum'], drop=drop)[:, 0]
    if not c['clamp01']:
        prob = _unclamped(p, x, c, drop)
    _pin(r['prob'], prob, r['S']['prob'], 'prob')
    for k, b in ((1, 1), (2, 5)):
        _pin(r['rm%d' % k], bn['readout_prob.fc.%d.running_mean' % b], r['S']['rm%d' % k], 'rm')
        _pin(r['rv%d' % k], bn['readout_prob.fc.%d.running_var' % b], r['S']['rv%d' % k], 'rv')
    (prob * c['dprob'].to(F64)).sum().backward()
    stats = torch.cat([r['stats1'], r['stats2']])
    b = RR.fused_bwd(c, r['y1'], r['y2'], stats, c['dprob'])
    _pin(b['dhf'], x.grad, b['S']['dhf'], 'dhf')
    names = {'dW1': 'fc.0.weight', 'db1': 'fc.0.bias', 'dgamma1': 'fc.1.weight', 'dbeta1': 'fc.1.bias', 'dW2': 'fc.4.weight', 'db2': 'fc.4.bias',
             'dgamma2': 'fc.5.weight', 'dbeta2': 'fc.5.bias', 'dw3': 'fc.8.weight', 'db3': 'fc.8.bias'}
    off = 0
    for k, n in RR.GRAD_BLOCKS:
        g = p['readout_prob.' + names[k]].grad.reshape(b[k].shape)
        _pin(b[k], g, b['S'][k], k)
        assert torch.equal(b['grads'][off:off + n], b[k].reshape(-1))
        off += n
    assert off == b['grads'].numel() == 3297


def _unclamped(p, x, c, drop):
    y = x
    for blk, (lin, bnl) in enumerate(((0, 1), (4, 5))):
        y = R.linear(p, 'readout_prob.fc.%d' % lin, y)
        y = F.batch_norm(y, None, None, p['readout_prob.fc.%d.weight' % bnl], p['readout_prob.fc.%d.bias' % bnl], training=True, eps=c['eps'])
        y = F.relu(y) * drop[blk]
    return R.linear(p, 'readout_prob.fc.8', y)[:, 0]


def test_momentum_keep_and_eps_away_from_the_defaults():
    """torch.nn.functional.batch_norm with momentum 0.3 and eps 1e-3, and keep = 1 - momentum given separately."""
    c = RR.fused_case(129, momentum=0.3, eps=1e-3)
    r = RR.fused_fwd_stages(c)
    y1 = r['y1']
    rm, rv = c['rm1'].to(F64).clone(), c['rv1'].to(F64).clone()
    bn = F.batch_norm(y1, rm, rv, c['g1'].to(F64), c['be1'].to(F64), training=True, momentum=0.3, eps=1e-3)
    _pin(r['rm1'], rm, r['S']['rm1'], 'rm1')
    _pin(r['rv1'], rv, r['S']['rv1'], 'rv1')
    xhat = (y1 - r['stats1'][:C]) * r['stats1'][C:]
    assert float((xhat * c['g1'].to(F64) + c['be1'].to(F64) - bn).abs().max()) <= 1e-9
    assert float(r['stats1'][C + RR.CONST_COL]) == pytest.approx(1e-3 ** -0.5, rel=1e-12) and c['keep'] == 0.7


def test_one_row_is_what_the_finalize_kernel_does():
    """N = 1: var = 0 in every column, invstd = rsqrt(eps), xhat = 0, bn = beta; the unbiased factor is N / max(N - 1, 1) = 1, so the
    running variance only decays (torch refuses one row in training mode; ops.BnReluDropFn guards the same way)."""
    c, r = _fused(1)
    assert torch.equal(r['stats1'][C:], torch.full((C,), RR.BN_EPS ** -0.5, dtype=F64))
    assert torch.allclose(r['rv1'], c['rv1'].to(F64) * c['keep'], rtol=1e-15)
    assert torch.allclose(r['rm1'], c['rm1'].to(F64) * c['keep'] + c['momentum'] * r['y1'][0], rtol=1e-12)
    assert torch.equal(r['bn1'][0], c['be1'].to(F64))
    k = RR.fused_fwd_stages(c, dtype=F32, mm='x3')
    assert RR.ratio(k['rv1'], r['rv1'], r['S']['rv1']) <= 2.0 ** -23


def test_chained_restatement_meets_the_reference_projects_fixtures():
    """g3_ops: the reference project's MLP in training mode (its float32 arithmetic: 1e-5 / 1e-4 relative as tests/test_oracle_golden.py);
    g1: its eval-mode readout from eval_hf to eval_prob through the per-layer restatements with the running statistics."""
    z = load_golden('g3_ops')
    q = {k: torch.from_numpy(z['mlp_param_' + k]) for k in ('fc.0.weight', 'fc.0.bias', 'fc.1.weight', 'fc.1.bias', 'fc.4.weight', 'fc.4.bias',
                                                           'fc.5.weight', 'fc.5.bias', 'fc.8.weight', 'fc.8.bias')}
    x, t = torch.from_numpy(z['mlp_in']), torch.from_numpy(z['mlp_target'])
    N = x.shape[0]
    c = {'N': N, 'hf': x, 'W1': q['fc.0.weight'], 'b1': q['fc.0.bias'], 'g1': q['fc.1.weight'], 'be1': q['fc.1.bias'], 'W2': q['fc.4.weight'],
         'b2': q['fc.4.bias'], 'g2': q['fc.5.weight'], 'be2': q['fc.5.bias'], 'w3': q['fc.8.weight'][0], 'b3': q['fc.8.bias'], 'p1': 0.0, 'p2': 0.0,
         'seed1': 1, 'seed2': 2, 'clamp01': 1, 'momentum': 0.1, 'keep': 0.9, 'eps': 1e-5, 'rm1': torch.zeros(C), 'rv1': torch.ones(C),
         'rm2': torch.zeros(C), 'rv2': torch.ones(C)}
    r = RR.fused_fwd_stages(c)
    np.testing.assert_allclose(r['prob'].numpy(), z['mlp_prob'].reshape(-1), rtol=1e-5, atol=1e-6)
    for k, b in ((1, 1), (2, 5)):
        np.testing.assert_allclose(r['rm%d' % k].numpy(), z['mlp_after_running_mean%d' % b], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(r['rv%d' % k].numpy(), z['mlp_after_running_var%d' % b], rtol=1e-5, atol=1e-6)
    l1 = RR.l1_fwd(r['prob'].to(F32), t.reshape(-1))
    np.testing.assert_allclose(float(l1['sum'][0]) / N, z['mlp_l1'], rtol=1e-5)
    dprob = RR.l1_bwd(r['prob'], t.reshape(-1).to(F64), 1.0)['dx']
    b = RR.fused_bwd(c, r['y1'], r['y2'], torch.cat([r['stats1'], r['stats2']]), dprob)
    np.testing.assert_allclose(b['dhf'].numpy(), z['mlp_grad_in'], rtol=1e-4, atol=1e-7)
    for k, n in (('dW1', 'fc.0.weight'), ('dgamma1', 'fc.1.weight'), ('dbeta1', 'fc.1.bias'), ('dW2', 'fc.4.weight'), ('dgamma2', 'fc.5.weight'),
                 ('dbeta2', 'fc.5.bias'), ('dw3', 'fc.8.weight'), ('db3', 'fc.8.bias')):
        np.testing.assert_allclose(b[k].numpy().reshape(z['mlp_grad_' + n].shape), z['mlp_grad_' + n], rtol=1e-4, atol=1e-6)

    z = load_golden('g1_aig')
    p = R.params_from_npz(z, requires_grad=False)
    P = lambda k: p['readout_prob.' + k]       # noqa: E731
    y = torch.from_numpy(z['eval_hf'])
    for lin, bn in ((0, 1), (4, 5)):
        y = (y.to(F64) @ P('fc.%d.weight' % lin).to(F64).t() + P('fc.%d.bias' % lin).to(F64)).to(F32)
        invstd = 1.0 / torch.sqrt(P('fc.%d.running_var' % bn).to(F64) + 1e-5)
        y = RR.bn_act_fwd(y, P('fc.%d.running_mean' % bn), invstd, P('fc.%d.weight' % bn), P('fc.%d.bias' % bn), 0.0, 5)['A'].to(F32)
    prob = RR.head_fwd(y, P('fc.8.weight')[0], P('fc.8.bias'), 1)['prob']
    np.testing.assert_allclose(prob.numpy(), z['eval_prob'].reshape(-1), rtol=5e-5, atol=2e-5)


# ------------------------------------------------------------------------------------------------ the builders
def test_band_is_eight_times_the_restatements_own_error():
    """BAND = the smallest power of ten >= 8 x the worst absolute pre-activation error of the float32 / 'x3' restatement against
    float64, over every builder case (per-layer and head cases at every width and size; the fused stages chained on given y1 / y2;
    the designed backward inputs)."""
    worst = {'relu': 0.0, 'head': 0.0}
    for Cw in RR.WIDTHS:
        for N in RR.layer_sizes(Cw):
            c = RR.layer_case(Cw, N)
            a = (c['Y'], c['mean'], c['invstd'], c['gamma'], c['beta'])
            worst['relu'] = max(worst['relu'], float((RR._bn(*a, F32)[2].to(F64) - RR._bn(*a, F64)[2]).abs().max()))
            h = RR.head_case(Cw, N)
            worst['head'] = max(worst['head'], float((RR._head(h['A'], h['w'], h['b'], F32)[0].to(F64) - RR._head(h['A'], h['w'], h['b'], F64)[0]).abs().max()))
    for N in RR.FUSED_SIZES:
        c, r = _fused(N)
        giv = {k: r[k].to(F32) for k in ('y1', 'stats1', 'y2', 'stats2')}
        r2 = RR.fused_fwd_stages(c, given=giv)
        k2 = RR.fused_fwd_stages(c, given=giv, dtype=F32, mm='x3', dec={q: r2[q] for q in ('relu1', 'relu2', 'inside')})
        y1, y2, st = RR.designed_bwd_inputs(c)
        for k, y, s in ((1, y1, st[:2 * C]), (2, y2, st[2 * C:])):
            a = (y, s[:C], s[C:], c['g%d' % k], c['be%d' % k])
            worst['relu'] = max(worst['relu'], float((RR._bn(*a, F32)[2].to(F64) - RR._bn(*a, F64)[2]).abs().max()))
        worst['relu'] = max(worst['relu'], float((k2['bn1'] - r2['bn1']).abs().max()), float((k2['bn2'] - r2['bn2']).abs().max()))
        worst['head'] = max(worst['head'], float((k2['h'] - r2['h']).abs().max()))
    w = max(worst.values())
    print('BAND: worst pre-activation error relu %.3g head %.3g -> 8 x = %.3g' % (worst['relu'], worst['head'], 8 * w))
    assert RR.BAND == 10.0 ** np.ceil(np.log10(8 * w)), (worst, RR.BAND)


@pytest.mark.parametrize('Cw', RR.WIDTHS)
def test_layer_builders_keep_their_promises(Cw):
    for N in RR.layer_sizes(Cw):
        c = RR.layer_case(Cw, N)
        a = (c['Y'], c['mean'], c['invstd'], c['gamma'], c['beta'])
        _, xhat, bn, _ = RR._bn(*a, F64)
        live = c['gamma'] != 0
        assert int(RR.banded(bn)[:, live].sum()) == 0                              # nudged: no entry may take either branch
        assert bool((bn[:, RR.DEAD_COL] < -RR.BAND).all())                         # all-dead ReLU
        assert bool((c['Y'][:, RR.CONST_COL] == 3.0).all()) and bool((xhat[:, RR.CONST_COL] == 0).all())
        assert float(c['invstd'][RR.CONST_COL]) == pytest.approx(RR.BN_EPS ** -0.5, rel=1e-6)
        assert float(c['gamma'][RR.ZERO_GAMMA_COL]) == 0.0
        if N >= 63:
            e = torch.log10(c['Y'][:, 0].abs().clamp(min=1e-30))
            assert float(e.max()) - float(e.min()) > 3                             # rows of very different magnitude
            if Cw >= 8:
                assert 0.02 < float((bn > 0).double().mean()) < 0.98                   # beta of either sign: columns mostly live, mostly dead
            assert N < 4099 or all(0 < int((bn[:, j] > 0).sum()) < N for j in range(Cw) if j not in (RR.CONST_COL, RR.ZERO_GAMMA_COL, RR.DEAD_COL))
        assert N == 1 or bool((c['dA'][N // 2] == 0).all())
        h = RR.head_case(Cw, N)
        hh, _ = RR._head(h['A'], h['w'], h['b'], F64)
        assert int(RR.banded(hh, (0.0, 1.0)).sum()) == 0
        assert N == 1 or float(h['dprob'][N // 2]) == 0.0


def test_fused_builders_keep_their_promises():
    for N in RR.FUSED_SIZES:
        c, r = _fused(N)
        for k in (1, 2):
            bn, live = r['bn%d' % k], c['g%d' % k] != 0
            assert bool((bn[:, RR.DEAD_COL] < -RR.BAND).all()), (N, k)
            assert int(RR.banded(bn)[:, live].sum()) <= RR.band_cap(N * C), (N, k)        # y2 / prob rows that may take either branch
            y = r['y%d' % k]
            assert bool((y[:, RR.CONST_COL] == y[0, RR.CONST_COL]).all())
            assert float(r['stats%d' % k][C + RR.CONST_COL]) == pytest.approx(RR.BN_EPS ** -0.5, rel=1e-9)
        assert int(RR.banded(r['h'], (0.0, 1.0)).sum()) <= RR.band_cap(N), N
        if N >= 63:
            assert 0.02 < float(r['inside'].double().mean()) < 0.98
        y1, y2, st = RR.designed_bwd_inputs(c)
        b = RR.fused_bwd(c, y1, y2, st, c['dprob'])
        assert int(RR.banded(b['bn1'])[:, c['g1'] != 0].sum()) == 0 and int(RR.banded(b['bn2'])[:, c['g2'] != 0].sum()) == 0, N
        assert int(RR.banded(b['h'], (0.0, 1.0)).sum()) == 0, N
        assert bool((b['bn1'][:, RR.DEAD_COL] < 0).all()) and bool((b['bn2'][:, RR.DEAD_COL] < 0).all())
        assert not torch.equal(y1.to(F64), r['y1'])
        # designed zeros come back as exact zeros
        assert float(b['dgamma1'][RR.DEAD_COL]) == 0 and float(b['dbeta2'][RR.DEAD_COL]) == 0
        assert float(b['dW1'][RR.ZERO_GAMMA_COL].abs().max()) == 0 and float(b['S']['dW1'][RR.ZERO_GAMMA_COL].abs().max()) == 0


def test_every_cap_edge_has_a_size_on_each_side():
    for k, (un, cap, u, cite) in RR.GEOMETRY.items():
        assert cite and cap in (512, 1024, 2048) and u in (1, 4)
    for Cw in (4, 32, 64):
        for k in ('colstats', 'bn_act_fwd', 'bn_act_bwd', 'bn_bwd_apply', 'head_fwd', 'head_bwd'):
            edge = RR.cap_rows(k, Cw)
            assert edge in RR.layer_sizes(Cw) and edge + 1 in RR.layer_sizes(Cw)
            assert RR.grid(k, edge, Cw) == RR.GEOMETRY[k][1] == -(-edge // RR.unit(k, Cw)) and -(-(edge + 1) // RR.unit(k, Cw)) == RR.grid(k, edge + 1, Cw) + 1
            assert max(n for n in RR.layer_sizes(Cw) if n < edge - 1) == 4099      # everything else below is far from the cap
    for k in ('l1_fwd', 'l1_bwd'):
        assert RR.cap_rows(k) in RR.L1_SIZES and RR.cap_rows(k) + 1 in RR.L1_SIZES
    for k in ('ro_fwd_lin', 'ro_b3', 'ro_db2', 'ro_head', 'ro_b1', 'ro_b2'):
        edge = RR.cap_rows(k)
        assert edge in RR.FUSED_SIZES and edge + 1 in RR.FUSED_SIZES, k
        assert -(-edge // RR.unit(k)) == RR.GEOMETRY[k][1] and RR.grid(k, edge + 1) == RR.GEOMETRY[k][1]
    # the partial U = 4 group: some thread holds 2 or 3 rows, another fewer; and the full group with a second outer pass
    r = RR.rows_per_wg(32)
    for k in ('bn_act_bwd', 'bn_bwd_apply'):
        assert RR.partial_u(k, 2 * RR.CAP * r + 7, 32) and RR.u_counts(k, 2 * RR.CAP * r + 7, 32) == (2, 3)
        assert RR.u_counts(k, 4 * RR.CAP * r + 5, 32) == (1, 1) and (4 * RR.CAP * r + 5 - 1) // (4 * RR.stride(k, 4 * RR.CAP * r + 5, 32)) == 1
        assert not any(RR.partial_u(k, n, 32) for n in RR.layer_sizes(32) if n <= RR.cap_rows(k, 32))
    for k in ('ro_b1', 'ro_b2'):
        assert RR.partial_u(k, 65536 + 128 * 3 + 5) and RR.u_counts(k, 65536 + 128 * 3 + 5) == (1, 2)
        assert RR.partial_u(k, 98305 + 64) and not RR.partial_u(k, 65536)
    # B3: two grids in one launch
    for n in RR.B3_SIZES[1:] + (65536, 98369):
        assert RR.grid('ro_b3', n) == 512 != RR.grid('ro_db2', n), n
    assert RR.grid('ro_b3', 32768) == RR.grid('ro_db2', 32768) == 512 and RR.grid('ro_db2', 32769) == 513 and RR.grid('ro_db2', 65537) == 1024
    t = -(-98369 // RR.TILE)
    assert sorted({len(range(b, t, 512)) for b in range(512)}) == [3, 4] and sorted({len(range(b, t, 1024)) for b in range(1024)}) == [1, 2]


# ------------------------------------------------------------------------------------------------ planted defects
def _far(r64, mut, rk, floors, only=None, why=''):
    """Every output the defect touches (`only`) is >= 10 x outside tau = 8 max(r, floor)."""
    tau = RR.taus(r64, rk, floors)
    got = RR.ratios(mut, r64)
    for k in only:
        print('DEFECT %s %s: %.3g of scale, tau %.3g' % (why, k, got[k], tau[k]))
        assert got[k] >= 10 * tau[k], (why, k, got[k], tau[k])


LAYER_FLOOR = {'sums': 'f32', 'dZ': 'f32', 'A': 'f32', 'dY': 'f32', 'prob': 'f32', 'dA': 'f32', 'dw': 'f32', 'db': 'f32', 'dx': 'f32', 'sum': 'f32'}


def _layer_runs(Cw, N, fn, args, **kw):
    r = fn(*args, **kw)
    dec = {k: r[k] for k in ('relu', 'inside') if k in r}
    return r, fn(*args, dtype=F32, dec=dec, **kw) if dec else fn(*args, dtype=F32, **kw)


@pytest.mark.parametrize('Cw,N', [(32, 33), (8, 4099), (32, 2 * RR.CAP * 32 + 7), (64, RR.CAP * 16 + 1)])
def test_planted_defects_in_the_per_layer_entries(Cw, N):
    c = RR.layer_case(Cw, N)
    a = (c['Y'], c['mean'], c['invstd'], c['gamma'], c['beta'], c['p'], c['seed'])
    last_wg = ((N - 1) // RR.rows_per_wg(Cw)) % RR.grid('colstats', N, Cw)
    capped = N > RR.cap_rows('colstats', Cw)
    Y = torch.full((N, Cw + 4), float('nan'))
    Y[:, :Cw] = c['Y']
    r, k = RR.colstats(Y, Cw + 4, Cw), RR.colstats(Y, Cw + 4, Cw, dtype=F32)
    fl = {'sums': 2.0 ** -53 * RR.chain_len('colstats', N, Cw)}
    _far(r, RR.colstats(Y, Cw + 4, Cw, mutate=('last_row',)), k, fl, ['sums'], 'colstats last row')
    if capped:
        _far(r, RR.colstats(Y, Cw + 4, Cw, mutate=('lost_wg', last_wg)), k, fl, ['sums'], 'colstats slab row')
    m = RR.colstats(Y, Cw + 4, Cw, mutate=('ld_ignored',))
    assert not bool(torch.isfinite(m['sums']).all()) or RR.ratios(m, r)['sums'] >= 10 * RR.taus(r, k, fl)['sums']

    r, k = _layer_runs(Cw, N, RR.bn_act_fwd, a)
    _far(r, RR.bn_act_fwd(*a, mutate=('last_row',)), k, LAYER_FLOOR, ['A'], 'bn_act_fwd last row')
    _far(r, RR.bn_act_fwd(*a, mutate=('mask_row4',)), k, LAYER_FLOOR, ['A'], 'mask index row*4+k')
    ab = a + (c['dA'],)
    r, k = _layer_runs(Cw, N, RR.bn_act_bwd, ab)
    _far(r, RR.bn_act_bwd(*ab, mutate=('last_row',)), k, LAYER_FLOOR, ['dZ', 'sums'], 'bn_act_bwd last row')
    _far(r, RR.bn_act_bwd(*ab, mutate=('swap',)), k, LAYER_FLOOR, ['sums'], 'dgamma / dbeta swapped')
    _far(r, RR.bn_act_bwd(*ab, mutate=('mask_row4',)), k, LAYER_FLOOR, ['dZ', 'sums'], 'bwd mask index')
    _far(r, RR.bn_act_bwd(*ab, mutate=('gate_on_y',)), k, LAYER_FLOOR, ['dZ', 'sums'], 'gate on y')
    if capped:
        _far(r, RR.bn_act_bwd(*ab, mutate=('lost_wg', last_wg)), k, LAYER_FLOOR, ['sums'], 'bn_act_bwd slab row')
    if RR.partial_u('bn_act_bwd', N, Cw):
        _far(r, RR.bn_act_bwd(*ab, mutate=('lost_u', -1)), k, LAYER_FLOOR, ['dZ', 'sums'], 'last partial u')
    for bs in (0, 1):
        ap = (c['Y'], c['mean'], c['invstd'], c['gamma'], c['dZ'], c['sums'], bs)
        r, k = RR.bn_bwd_apply(*ap), RR.bn_bwd_apply(*ap, dtype=F32)
        _far(r, RR.bn_bwd_apply(*ap, mutate=('last_row',)), k, LAYER_FLOOR, ['dY'], 'apply last row')
        if bs == 0:
            _far(r, RR.bn_bwd_apply(*ap, mutate=('eval_keeps_correction',)), k, LAYER_FLOOR, ['dY'], 'correction kept in eval mode')
        else:
            _far(r, RR.bn_bwd_apply(*ap, mutate=('no_invstd_a2',)), k, LAYER_FLOOR, ['dY'], 'invstd left out of a2')
            if RR.partial_u('bn_bwd_apply', N, Cw):
                _far(r, RR.bn_bwd_apply(*ap, mutate=('lost_u', -1)), k, LAYER_FLOOR, ['dY'], 'apply last partial u')

    h = RR.head_case(Cw, N)
    ha = (h['A'], h['w'], h['b'], 1)
    r, k = _layer_runs(Cw, N, RR.head_fwd, ha)
    _far(r, RR.head_fwd(*ha, mutate=('last_row',)), k, LAYER_FLOOR, ['prob'], 'head last row')
    _far(r, RR.head_fwd(*ha, mutate=('dpp_short',)), k, LAYER_FLOOR, ['prob'], 'DPP sum one step short')
    hb = ha + (h['dprob'],)
    r, k = _layer_runs(Cw, N, RR.head_bwd, hb)
    _far(r, RR.head_bwd(*hb, mutate=('last_row',)), k, LAYER_FLOOR, ['dA', 'dw', 'db'], 'head_bwd last row')
    _far(r, RR.head_bwd(*hb, mutate=('db_col',)), k, LAYER_FLOOR, ['db'], 'db from slab column C - 1')
    _far(r, RR.head_bwd(*hb, mutate=('clamp_open_above',)), k, LAYER_FLOOR, ['dA', 'dw', 'db'], 'clamp gate open above 1')
    if capped:
        _far(r, RR.head_bwd(*hb, mutate=('lost_wg', last_wg)), k, LAYER_FLOOR, ['dw', 'db'], 'head slab row')


def test_planted_defects_in_the_l1_entries():
    """mgv_l1_loss_fwd is judged against S + |a0| with |a0| <= S (the device test's pre-filled accumulator), so a defect has to stand
    20 x tau above S alone.  At every size the last element lost; at 257 the slab row of workgroup 1 (that element alone); one past the
    cap and at two caps + 3 the second visit (one element; a whole visit)."""
    for n in RR.L1_SIZES:
        c = RR.l1_case(n)
        assert not bool(c['tie'][n - 1]) and float((c['x'][n - 1] - c['t'][n - 1]).abs()) > 90 and (n < 4 or int(c['tie'].sum()) >= n // 4 - 1)
        r, k = RR.l1_fwd(c['x'], c['t']), RR.l1_fwd(c['x'], c['t'], dtype=F32)
        tau = RR.taus(r, k, LAYER_FLOOR)['sum']
        plant = [('last_row',), ('lost_wg', ((n - 1) // RR.THREADS) % RR.grid('l1_fwd', n))]
        if n > RR.cap_rows('l1_fwd'):
            plant.append(('lost_visit', 1))
        for m in plant:
            got = RR.ratios(RR.l1_fwd(c['x'], c['t'], mutate=m), r)['sum']
            print('DEFECT l1_fwd n=%d %s sum: %.3g of scale, tau %.3g' % (n, m, got, tau))
            assert got >= 20 * tau, (n, m, got, tau)
        r, k = RR.l1_bwd(c['x'], c['t'], -0.37), RR.l1_bwd(c['x'], c['t'], -0.37, dtype=F32)
        assert RR.ratios(RR.l1_bwd(c['x'], c['t'], -0.37, mutate=('tie_positive',)), r)['dx'] == (float('inf') if bool(c['tie'].any()) else 0.0)
        _far(r, RR.l1_bwd(c['x'], c['t'], -0.37, mutate=('last_row',)), k, LAYER_FLOOR, ['dx'], 'l1_bwd last row')


@pytest.mark.parametrize('N', [63, 32769, 65536 + 128 * 3 + 5])
def test_planted_defects_in_the_fused_entries(N):
    c, r = _fused(N)
    dec = {q: r[q] for q in ('relu1', 'relu2', 'inside')}
    k = RR.fused_fwd_stages(c, dtype=F32, mm='x3', dec=dec)
    fw = lambda m: RR.fused_fwd_stages(c, mutate=m)       # noqa: E731
    _far(r, fw(('last_row',)), k, RR.FWD_FLOOR, ['y1', 'y2', 'prob'], 'fused last row')
    _far(r, fw(('biased_var',)), k, RR.FWD_FLOOR, ['rv1', 'rv2'] if N < 1000 else [], 'biased running variance')
    _far(r, fw(('swap_momentum_keep',)), k, RR.FWD_FLOOR, ['rm1', 'rv1', 'rm2', 'rv2'], 'momentum and keep swapped')
    _far(r, fw(('mask1_for_2',)), k, RR.FWD_FLOOR, ['prob'], 'mask of layer 1 in layer 2')
    _far(r, fw(('dpp_short',)), k, RR.FWD_FLOOR, ['prob'], 'DPP sum one step short')
    if N > RR.cap_rows('ro_fwd_lin'):
        wg = ((N - 1) // RR.TILE) % RR.grid('ro_fwd_lin', N)
        _far(r, fw(('lost_wg', wg)), k, RR.FWD_FLOOR, ['stats1', 'rm1', 'rv1'], 'statistics slab row')

    for tag, (y1, y2, st) in (('own', (r['y1'].to(F32), r['y2'].to(F32), torch.cat([r['stats1'], r['stats2']]).to(F32))), ('designed', RR.designed_bwd_inputs(c))):
        b = RR.fused_bwd(c, y1, y2, st, c['dprob'])
        kb = RR.fused_bwd(c, y1, y2, st, c['dprob'], dtype=F32, mm='x3', dec={q: b[q] for q in ('relu1', 'relu2', 'inside')})
        bw = lambda m: RR.fused_bwd(c, y1, y2, st, c['dprob'], mutate=m)       # noqa: E731
        _far(b, bw(('last_row',)), kb, RR.BWD_FLOOR, ['dhf'], tag + ' bwd last row')
        _far(b, bw(('db_col',)), kb, RR.BWD_FLOOR, ['db3'], tag + ' db3 from slab column C - 1')
        _far(b, bw(('swap',)), kb, RR.BWD_FLOOR, ['dgamma2', 'dbeta2'], tag + ' dgamma2 / dbeta2 swapped')
        _far(b, bw(('mask1_for_2',)), kb, RR.BWD_FLOOR, ['dhf', 'dw3', 'dgamma2'], tag + ' mask of layer 1 in layer 2')
        _far(b, bw(('gate_on_y',)), kb, RR.BWD_FLOOR, ['dhf', 'dgamma1', 'dgamma2'], tag + ' gate on y')
        _far(b, bw(('no_invstd_a2',)), kb, RR.BWD_FLOOR, ['dhf'], tag + ' invstd left out of a2')
        _far(b, bw(('clamp_open_above',)), kb, RR.BWD_FLOOR, ['dhf', 'dw3', 'db3'], tag + ' clamp gate open above 1')
        _far(b, bw(('dpp_short',)), kb, RR.BWD_FLOOR, ['dw3', 'db3'], tag + ' DPP sum one step short')
        if N > RR.cap_rows('ro_b1'):
            wg = (int((c['dprob'].abs() * b['inside']).argmax()) // 32) % RR.grid('ro_b1', N)        # the workgroup of the largest dy
            _far(b, bw(('lost_wg', wg)), kb, RR.BWD_FLOOR, ['dw3', 'db3', 'dgamma2', 'dbeta2'], tag + ' B1 slab row')
            _far(b, bw(('lost_u', -1)), kb, RR.BWD_FLOOR, ['dw3', 'db3', 'dgamma2', 'dbeta2'], tag + ' B1 last partial u')
        # (at 513 tiles the second set holds the last row alone: the forward's own last row is clamped away, the designed one is not)
        if RR.grid('ro_db2', N) > RR.grid('ro_b3', N) + (1 if tag == 'own' else 0):
            _far(b, bw(('db2_g3n',)), kb, RR.BWD_FLOOR, ['db2'], tag + ' db2 from g3n workgroups only')


# ------------------------------------------------------------------------------------------------ refusals on the host
def test_unserved_widths_and_sizes_are_refused_on_the_host_before_anything_is_launched():
    """c_ok, ld, p_drop and N are looked at before any pointer is read or anything is launched, so this runs without a GPU (the
    pointers are dummies).  The same on the device, with real buffers that must come back untouched: tests/test_hip_readout_entries.py."""
    import ctypes
    from deepgate import _hip
    lib, sigs = _hip.load(), _hip.parse_header()
    dummy = ctypes.c_void_p(64)

    def rc(name, **kw):
        import re
        with open(_hip.HEADER_PATH) as f:
            text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
        decl = re.search(r'\bint\s+%s\s*\(([^;]*?)\)\s*;' % name, text, flags=re.S).group(1)
        names = [a.strip().split()[-1].lstrip('*') for a in decl.split(',')]
        args = []
        for n, t in zip(names, sigs[name]):
            v = kw.get(n, dummy if t is ctypes.c_void_p else (0.25 if t is ctypes.c_float else (32 if n in ('C', 'ld') else (1 << 30 if n == 'workspace_doubles' else 8))))
            args.append(v)
        args[-1] = None
        return getattr(lib, name)(*args)

    layer = ('mgv_colstats', 'mgv_bn_act_fwd', 'mgv_bn_act_bwd', 'mgv_bn_bwd_apply', 'mgv_readout_head_fwd', 'mgv_readout_head_bwd')
    for name in layer:
        for Cw in (0, 1, 2, 3, 12, 24, 48, 128, -4):
            assert rc(name, C=Cw, ld=max(Cw, 4)) == -1, (name, Cw)
        assert rc(name, N=-1) == -1, name
        assert rc(name, N=0) == 0, name                               # nothing to do: success, nothing launched
    for ld in (28, 31, 34):
        assert rc('mgv_colstats', ld=ld) == -1, ld
    for p in (1.0, -0.1, 1.5):
        assert rc('mgv_bn_act_fwd', p_drop=p) == -1 and rc('mgv_bn_act_bwd', p_drop=p) == -1, p
    for name in ('mgv_l1_loss_fwd', 'mgv_l1_loss_bwd'):
        assert rc(name, n=-1) == -1 and rc(name, n=0) == 0
    for name in ('mgv_readout_fused_fwd', 'mgv_readout_fused_bwd'):
        assert rc(name, N=0) == -1 and rc(name, N=-1) == -1
        for p in (1.0, -0.1):
            assert rc(name, p1=p) == -1 and rc(name, p2=p) == -1
        assert rc(name, N=64, workspace_doubles=RR.ws_doubles(64) - 1) == -1
    assert _hip.call_value('mgv_readout_fused_pack_elems') == 2 * (2 * C * D + 2 * C * C)
    assert _hip.call_value('mgv_readout_fused_grad_floats') == sum(n for _, n in RR.GRAD_BLOCKS)
    assert _hip.call_value('mgv_sum_workspace_doubles') >= RR.CAP * 2 * 64                 # the widest served C at the grid cap
    for N in RR.FUSED_SIZES + (0, 1 << 20):
        assert _hip.call_value('mgv_readout_fused_ws_doubles', N) == RR.ws_doubles(N), N
