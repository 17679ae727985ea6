"""The training-mode readout WITH DROPOUT ON against a float64 reference that is not built from our kernels.

The device's dropout mask is a counter-based hash of (seed, element) (csrc/mgv_dropout.h); `oracle.ref_cpu.drop_factors` restates it
on the CPU (tests/test_dropout_mask_spec.py), and `oracle.ref_cpu.readout_prob(drop=...)` takes the restated factors in place of
`F.dropout`.  Here:

1. `test_device_mask_is_the_restated_mask`: the restatement is tied to the device bit for bit (`ops.BnReluDropFn`, BatchNorm output
   positive everywhere, so the zeros of the output are the mask), and the kept entries are bn_out / (1 - p).
2. `test_readout_against_float64_reference`: both readout paths (fused `ops.ReadoutMLPFn`, per-layer `linear / BnReluDropFn / HeadFn`)
   at p = 0.2, p = 0.5 and p = (0.2, 0.5), two upstream gradients (the product's L1 loss; `(prob * w).sum()` with random w):
   forward free-running, the device's piecewise-linear decisions counted against the reference's own, every gradient on the device's
   branches; the per-layer activations are zero wherever the restated mask drops.
3. `test_one_hot_upstream_through_bn_relu_drop`: forward and backward regenerate the SAME mask: a one-hot upstream on a dropped unit
   gives dy = 0 everywhere, on a kept one 1/(1-p) times the BatchNorm backward of that one-hot.
4. `test_train_step_at_the_product_dropout_against_the_oracle`: one whole `Trainer.run_batch` at the model's default p_drop = 0.2,
   weights [1, 4, 4], against the float64 oracle with the restated masks.

Grid-stride coverage at N = 1 << 20 (launch caps read from the launchers; 256 CUs x per-CU factor): the per-layer element-wise kernels
(`ew_grid`, cap 2048 workgroups of 256 float4s) see 32768 workgroups of work, 16 trips (4 in `k_bn_bwd_apply`, which keeps 4 in flight);
the row kernels (`k_colstats`, `k_bn_act_bwd`, `k_head`: 32 rows per workgroup, cap 2048) 16 trips (4 in `k_bn_act_bwd`); `k_l1_*` 2 trips;
the fused tile kernels see 16384 tiles of 64 rows against caps of 1024 (forward), 512 (B3) and 1024 (its db2 set): 16, 32 and 16 trips;
the fused row passes B1, B2 and the head (cap 2048, 4 groups of 32 rows in flight) 4 trips.  Every slab reduction (`k_slab_sum`) then adds
2048 (512, 1024) rows, 16 per phase in steps of 128: more than one trip of both of its loops.  At N <= 4099 every grid is uncapped and each
loop runs once, with the ragged last tile / row group at 63, 65 and 4099.

Bounds.  Ceilings from the project's own numbers: 1e-4 of scale for bf16x3 forward values and running buffers against float64
(test_hip_linear_x3.py), 1e-3 of scale for gradients on imposed branches (smoke(), x3 mode; 1e-4 in f32 mode).  Rule: where the worst
measured ratio over the parametrisation is under a quarter of the ceiling, the bound is 4 x that worst (the kernels are
bit-reproducible: the margin is for a compiler changing contraction or summation order), else the ceiling.

MEASURED on an MI355X, bf16x3 mode, worst over p, upstream and N (error / largest entry of the float64 tensor; per-layer and fused give
the same figures to the digits shown, they agree with each other to 1e-5; full table in NOTEBOOK.md, 2026-10-16):
    prob                      3.2e-5   (N = 2^20, p = 0.5)                      -> bound 1e-4 (ceiling)
    running mean / var        4.7e-6   (fc.5.running_mean, N = 2)               -> bound 1.9e-5
    gradients, N >= 63        1.56e-5  (fc.1.bias at N = 2^20; dhf 1.0e-5)      -> bound 6.3e-5
    gradients, N = 2          6.2e-4   (fc.1.weight; dhf 4.5e-4)                -> bound 1e-3 (ceiling)
Two rows get a bound of their own because they are another regime: the BatchNorm backward over two rows cancels to a residue of order
eps / var of its input gradient, every gradient behind BN2 is that residue, and the bf16x3 error of the linear outputs shows 40 x
larger against it (exact-fp32 mode, per-layer path: 2.8e-5 at N = 2, 4.0e-6 from 63 on); one bound over all N would have left the
N >= 63 cases at the ceiling.
Decision flips, worst per N, both paths: 0 up to N = 65, 1 at 4099 (cap 27), 93 at 2^20 (cap 6,920); cap max(4, 1e-4 x (64 N + 2 N)).
Whole train step: 0 flips; worst gradient 3.3e-5 of scale (bound 1e-3).
"""
import copy
import functools
import types

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the package on the path)
from test_hip_readout_fused import _inputs, _mlp

pytestmark = pytest.mark.gpu

# ceilings (never to be raised) and the bounds in force: 4 x the measured worst where that is under a quarter of the ceiling
CEIL_FWD, CEIL_GRAD_X3, CEIL_GRAD_F32 = 1e-4, 1e-3, 1e-4
BOUND_PROB = CEIL_FWD               # measured worst 3.2e-5: not under a quarter
BOUND_BUF = 1.9e-5                  # measured worst 4.7e-6
BOUND_GRAD_X3_TWO_ROWS = CEIL_GRAD_X3      # N = 2, measured worst 6.2e-4: not under a quarter
BOUND_GRAD_X3 = 6.3e-5              # N >= 63, measured worst 1.56e-5

P_CASES = {'p0.2': (0.2, 0.2, 1234), 'p0.5': (0.5, 0.5, 2 ** 62 - 5), 'p0.2-0.5': (0.2, 0.5, 4242)}      # p layer 1, p layer 2, seed
NS = (2, 63, 64, 65, 4099, 1 << 20)
PFX = 'readout_prob.'


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _grad_bound(N):
    from deepgate import ops
    if ops.PRECISION == 'f32':
        return CEIL_GRAD_F32
    return BOUND_GRAD_X3_TWO_ROWS if N == 2 else BOUND_GRAD_X3


def _flip_cap(N):
    return max(4, int(1e-4 * (64 * N + 2 * N)))


def _measure(**kv):
    print('\nMEASURE ' + ' '.join('%s=%s' % (k, ('%.3e' % v) if isinstance(v, float) else v) for k, v in kv.items()))


# ------------------------------------------------------------------------------------------------ 1. the mask, device against CPU
@pytest.mark.parametrize('seed', [7, 2 ** 62 - 5])
@pytest.mark.parametrize('p', [0.1, 0.2, 0.5])
@pytest.mark.parametrize('N', [1, 63, 64, 65, 4099])
@pytest.mark.parametrize('C', [32, 8, 64])
def test_device_mask_is_the_restated_mask(C, N, p, seed):
    dev = _dev()
    from deepgate import ops
    from oracle import ref_cpu as R
    g = torch.Generator().manual_seed(100 * C + N)
    y = torch.randn(N, C, generator=g)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.full((C,), 10.0)
    y64 = y.double()
    mean, var = y64.mean(0), y64.var(0, unbiased=False)
    bn = (y64 - mean) / torch.sqrt(var + 1e-5) * gamma.double() + beta.double()
    assert float(bn.min()) > 1.0                                   # the ReLU passes everything: the output's zeros are the mask's
    a = ops.BnReluDropFn.apply(y.to(dev), gamma.to(dev), beta.to(dev), torch.zeros(C, device=dev), torch.ones(C, device=dev),
                               True, p, seed, 0.1, 1e-5).cpu()
    f = R.drop_factors(seed, N, C, p)
    assert torch.equal(a != 0, f != 0), int(((a != 0) != (f != 0)).sum())
    want = bn * f
    # float32 roundings on the way: the subtraction, two products, the sum, the factor, and invstd's own (a float32 rsqrt of the
    # float64 variance): under ten roundings of 2^-24 relative to the largest entry
    err = float((a.double() - want).abs().max()) / float(want.abs().max())
    assert err <= 1e-6, err
    assert torch.equal(a == 0, f == 0)


# ------------------------------------------------------------------------------------------------ 2. both paths against float64
def _run_device(base, hf, up, fused, seed, capture=False):
    """One forward + backward of a copy of `base` on the device.  up = ('l1', target) or ('wsum', w)."""
    from deepgate import ops
    from deepgate.arch import mlp as mlp_mod
    m = copy.deepcopy(base)
    relu = []
    old_flag, bn_apply = mlp_mod.FUSED_READOUT, ops.BnReluDropFn.apply
    mlp_mod.FUSED_READOUT = fused
    if capture:
        def bn_capture(*a):
            out = bn_apply(*a)
            relu.append(out.detach().cpu())
            return out
        ops.BnReluDropFn.apply = bn_capture
    try:
        x = hf.clone().requires_grad_(True)
        prob = m(x, clamp01=True, seed=seed)
        node = type(prob.grad_fn).__name__
        loss = ops.l1_loss(prob, up[1]) if up[0] == 'l1' else (prob * up[1]).sum()
        loss.backward()
    finally:
        mlp_mod.FUSED_READOUT = old_flag
        ops.BnReluDropFn.apply = bn_apply
    torch.cuda.synchronize()
    assert ('ReadoutMLPFn' in node) == bool(fused), node          # the path asked for is the path that ran
    out = {'prob': prob.detach().cpu(), 'dhf': x.grad.detach().cpu(), 'act': relu,
           'grads': {k: q.grad.detach().cpu() for k, q in m.named_parameters()},
           'bufs': {k: v.detach().cpu() for k, v in m.state_dict().items() if 'running' in k}}
    return out


def _oracle_params(base):
    p = {}
    for k, v in base.state_dict().items():
        v = v.detach().cpu()
        if v.is_floating_point():
            v = v.double()
            if 'running_' not in k:
                v.requires_grad_(True)
        p[PFX + k] = v
    return p


def _upstream(kind, N, target, dev):
    if kind == 'l1':
        return ('l1', target)
    w = torch.randn(N, 1, generator=torch.Generator().manual_seed(N + 17))
    return ('wsum', w.to(dev))


@functools.lru_cache(maxsize=1)
def _case(pcase, N, kind):
    """The per-layer device run (its decisions captured) and the float64 reference of one (p, N, upstream) case: free-running, and
    again on the device's branches with gradients.  Cached for the two paths that are held to it."""
    from oracle import ref_cpu as R
    dev = _dev()
    p1, p2, seed = P_CASES[pcase]
    hf, target = _inputs(N, dev)
    base = _mlp(p1, dev)
    base.fc[7].p = p2
    up = _upstream(kind, N, target, dev)
    d = _run_device(base, hf, up, False, seed, capture=True)
    assert len(d['act']) == 2
    drop = [R.drop_factors(seed, N, 32, p1), R.drop_factors(seed + 7919, N, 32, p2)]
    par = _oracle_params(base)
    hf64 = hf.cpu().double()
    t64, u64 = target.cpu().double(), up[1].cpu().double()
    # free-running: its own ReLU and clamp decisions
    bn_free = {k: v.clone() for k, v in par.items() if 'running_' in k}
    own = {}
    with torch.no_grad():
        prob_free = R.readout_prob(par, hf64, True, bn_free, drop=drop, taken=own)
    ref = {'prob': prob_free, 'bufs': {k[len(PFX):]: v for k, v in bn_free.items()}, 'own': own, 'drop': drop, 'target': t64, 'up': u64}
    # the device's decisions (per-layer path): ReLU masks on the kept elements, clamp mask, L1 signs
    dec = {'relu': [a > 0 for a in d['act']], 'inside': (d['prob'] > 0) & (d['prob'] < 1)}
    ref['dec'] = dec
    x = hf64.clone().requires_grad_(True)
    prob_imp = R.readout_prob(par, x, True, {k: v.clone() for k, v in par.items() if 'running_' in k}, decisions=dec, drop=drop)
    if kind == 'l1':
        loss = (torch.sign(d['prob'].double() - t64) * (prob_imp - t64)).mean()
    else:
        loss = (prob_imp * u64).sum()
    loss.backward()
    ref['grads'] = {k[len(PFX):]: v.grad for k, v in par.items() if v.requires_grad}
    ref['dhf'] = x.grad
    return base, hf, up, d, ref


def _count_flips(act, prob, ref, kind):
    """Decisions of a device run (ReLU: the kept elements of the per-layer activations `act`; clamp and L1 signs: its `prob`) that
    differ from the float64 reference's own."""
    own, drop = ref['own'], ref['drop']
    flips = sum(int((((act[k] > 0) != own['relu'][k]) & (drop[k] != 0)).sum()) for k in range(2))
    y = own['pre_clamp']
    flips += int((((prob > 0) & (prob < 1)) != ((y > 0) & (y < 1))).sum())
    if kind == 'l1':
        flips += int((torch.sign(prob.double() - ref['target']) != torch.sign(ref['prob'] - ref['target'])).sum())
    return flips


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'perlayer'])
@pytest.mark.parametrize('kind', ['l1', 'wsum'])
@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('pcase', list(P_CASES))
def test_readout_against_float64_reference(pcase, N, kind, fused):
    from deepgate import ops
    _dev()
    if fused and ops.PRECISION != 'x3':
        pytest.skip('the fused readout is bf16x3 only')
    p1, p2, seed = P_CASES[pcase]
    base, hf, up, d_pl, ref = _case(pcase, N, kind)
    d = _run_device(base, hf, up, True, seed) if fused else d_pl
    tag = dict(path='fused' if fused else 'perlayer', p=pcase, N=N, up=kind)

    # the per-layer activations are zero wherever the restated mask drops, in both layers (the mask of layer 2 is layer 2's)
    for k in range(2):
        assert not bool(((d_pl['act'][k] != 0) & (ref['drop'][k] == 0)).any()), 'layer %d: a dropped unit is live' % (k + 1)

    # forward, free-running
    err = float((d['prob'].double() - ref['prob']).abs().max()) / max(float(ref['prob'].abs().max()), 1e-30)
    _measure(tensor='prob', err=err, **tag)
    worst_buf = 0.0
    for k, r in ref['bufs'].items():
        e = float((d['bufs'][k].double() - r).abs().max()) / float(r.abs().max())
        worst_buf = max(worst_buf, e)
        _measure(tensor=k, err=e, **tag)

    # decisions, counted (the fused path keeps no activations: its clamp mask and L1 signs are its own, its ReLU decisions are the
    # per-layer path's, which test_hip_readout_fused.py holds it to)
    flips = _count_flips(d_pl['act'], d['prob'], ref, up[0])
    if fused:
        # the reference's gradient below is formed on the per-layer run's branches: the fused run must have taken the same ones
        assert torch.equal((d['prob'] > 0) & (d['prob'] < 1), ref['dec']['inside']), 'the two paths clamp different rows'
        if up[0] == 'l1':
            t = up[1].cpu()
            assert torch.equal(torch.sign(d['prob'] - t), torch.sign(d_pl['prob'] - t)), 'the two paths take different L1 signs'
    _measure(tensor='flips', count=flips, cap=_flip_cap(N), **tag)

    # backward, on the device's branches
    gerr = {}
    gref = ref['grads']
    for k, r in list(gref.items()) + [('dhf', ref['dhf'])]:
        g = d['dhf'] if k == 'dhf' else d['grads'][k]
        scale = float(r.abs().max())
        if k in ('fc.0.bias', 'fc.4.bias'):
            # a bias in front of a BatchNorm: mathematically zero gradient, priced against its layer's weight gradient
            scale = max(scale, float(gref[k.replace('bias', 'weight')].abs().max()))
        gerr[k] = float((g.double() - r).abs().max()) / max(scale, 1e-300)
        _measure(tensor=k, err=gerr[k], scale=scale, **tag)

    assert err <= BOUND_PROB, ('prob', err)
    assert worst_buf <= BOUND_BUF, ('running buffers', worst_buf)
    assert flips <= _flip_cap(N), ('decision flips', flips, _flip_cap(N))
    bad = {k: v for k, v in gerr.items() if not v <= _grad_bound(N)}
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 3. one mask, forward and backward
@pytest.mark.parametrize('p', [0.2, 0.5])
@pytest.mark.parametrize('C', [32, 8])
def test_one_hot_upstream_through_bn_relu_drop(C, p):
    """dy of `BnReluDropFn` for a one-hot upstream at (i, c), BatchNorm output positive everywhere.  Unit dropped in the forward (restated
    mask 0): dz = 0, so dy is zero in every row, exactly.  Unit kept: dy = 1/(1-p) x the BatchNorm backward of the one-hot, column c
    only.  The units are picked at the first and last rows, across a 4-row boundary of the backward's in-flight groups, and at large
    element numbers, dropped and kept ones of each."""
    dev = _dev()
    from deepgate import ops
    from oracle import ref_cpu as R
    N, seed = 4099, 2 ** 62 - 5
    g = torch.Generator().manual_seed(C)
    y = torch.randn(N, C, generator=g)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.full((C,), 10.0)
    f = R.drop_factors(seed, N, C, p)
    yd = y.to(dev).requires_grad_(True)
    a = ops.BnReluDropFn.apply(yd, gamma.to(dev), beta.to(dev), torch.zeros(C, device=dev), torch.ones(C, device=dev), True, p, seed, 0.1, 1e-5)
    assert torch.equal(a.detach().cpu() != 0, f != 0)
    y64 = y.double().requires_grad_(True)
    bn = torch.nn.functional.batch_norm(y64, None, None, gamma.double(), beta.double(), training=True, eps=1e-5)
    assert float(bn.detach().min()) > 1.0
    rows = [0, 1, 31, 32, 33, 127, 128, 2048, 4097, 4098]
    seen = {True: 0, False: 0}
    for i in rows:
        for c in (0, 3, C - 1):
            kept = bool(f[i, c] != 0)
            seen[kept] += 1
            up = torch.zeros(N, C)
            up[i, c] = 1.0
            dy, = torch.autograd.grad(a, yd, up.to(dev), retain_graph=True)
            dy = dy.cpu()
            if not kept:
                assert float(dy.abs().max()) == 0.0, (i, c)
                continue
            want, = torch.autograd.grad(bn, y64, up.double(), retain_graph=True)
            want = want / (1.0 - float(np.float32(p)))
            off = torch.ones(C, dtype=torch.bool)
            off[c] = False
            assert float(dy[:, off].abs().max()) == 0.0, (i, c)
            err = float((dy.double() - want).abs().max()) / float(want.abs().max())
            assert err <= 1e-5, (i, c, err)          # fp32 element-wise kernel against float64: a few roundings of 6e-8
    assert seen[True] >= 5 and seen[False] >= 3, seen


# ------------------------------------------------------------------------------------------------ 4. one whole train step, p_drop = 0.2
@pytest.mark.parametrize('ctype', ['aig', 'xmg'])
def test_train_step_at_the_product_dropout_against_the_oracle(ctype):
    """`Trainer.run_batch` with the model as the product builds it (p_drop = 0.2 in the readout, dim_hidden 64: the fused readout node),
    weights [1, 4, 4], three synthetic graphs; the oracle runs in float64 with the restated masks.  The per-layer path runs first and
    gives the ReLU decisions; both paths are then held to the oracle on those branches at the bounds of
    test_hip_model.test_other_hidden_widths_against_the_oracle, and the decisions are counted against the oracle's own."""
    dev = _dev()
    import deepgate
    from deepgate import ops, synthetic as syn
    from deepgate.arch import mlp as mlp_mod
    from oracle import ref_cpu as R
    from test_hip_model import close, grad_atol
    H, SEED, W = 64, 31337, [1.0, 4.0, 4.0]
    torch.manual_seed(5)
    enc = deepgate.digae_layer.DirectMultiGCNEncoder(dim_feature=6, dim_hidden=H, s_rounds=2, t_rounds=2, layernorm=True)
    model = getattr(deepgate, 'dg_ae_model_' + ctype).Model(struct_encoder=enc, dim_hidden=H)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, (torch.nn.LayerNorm, torch.nn.BatchNorm1d)):
                m.weight.add_(0.2 * torch.randn_like(m.weight)); m.bias.add_(0.2 * torch.randn_like(m.bias))
    drops = [m for m in model.readout_prob.modules() if isinstance(m, torch.nn.Dropout)]
    assert [m.p for m in drops] == [0.2, 0.2]                       # the product's default, untouched
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model.to(dev).train()
    arrays = syn.collate([syn.make_graph(ctype, 150, 6, 600 + i, n_inputs=12) for i in range(3)])
    batch = deepgate.CircuitBatch.from_arrays(arrays, device=dev)
    N = batch.x.shape[0]
    tr = deepgate.Trainer(types.SimpleNamespace(model='DG_AE'), model, training_id='drop', save_dir='/tmp/mgv_test_exp', lr=1e-4,
                          rc_prob_func_weight=W, device='cuda:0', batch_size=3, distributed=False)

    def device_step(fused):
        model.load_state_dict(sd)
        tr.optimizer.zero_grad()
        got = {'relu': []}
        old_flag, bn_apply, head = mlp_mod.FUSED_READOUT, ops.BnReluDropFn.apply, model.pred_prob

        def bn_capture(*a):
            out = bn_apply(*a)
            got['relu'].append(out.detach().cpu())
            return out

        def seeded(hf, seed=None):
            out = head(hf, seed=SEED)
            got['prob'], got['node'] = out.detach().cpu(), type(out.grad_fn).__name__
            return out
        mlp_mod.FUSED_READOUT, ops.BnReluDropFn.apply, model.pred_prob = fused, bn_capture, seeded
        try:
            ls = tr.run_batch(batch)
            tr.weighted_loss(ls).backward()
        finally:
            mlp_mod.FUSED_READOUT, ops.BnReluDropFn.apply = old_flag, bn_apply
            del model.pred_prob
        torch.cuda.synchronize()
        got['losses'] = {k: float(ls[k].detach()) for k in ('recon_loss', 'prob_loss', 'func_loss')}
        got['grads'] = {k: (None if q.grad is None else q.grad.detach().cpu().clone()) for k, q in model.named_parameters()}
        return got

    per_layer = device_step(False)
    assert len(per_layer['relu']) == 2 and 'HeadFn' in per_layer['node']
    runs = {'perlayer': per_layer}
    if ops.PRECISION == 'x3':
        runs['fused'] = device_step(True)
        assert 'ReadoutMLPFn' in runs['fused']['node'] and not runs['fused']['relu']

    drop = [R.drop_factors(SEED, N, 32, 0.2), R.drop_factors(SEED + 7919, N, 32, 0.2)]
    ob = R.batch_from_arrays(lambda k: arrays[k])
    label = ob['prob'].double()

    def oracle(decisions, taken=None):
        p = {k: ((v.clone().double().requires_grad_(True) if 'running_' not in k else v.clone().double()) if v.is_floating_point() else v.clone())
             for k, v in sd.items()}
        bn = {k: v.clone() for k, v in p.items() if 'running_' in k}
        ols = R.run_batch(p, ctype, ob, training=True, bn_state=bn, s_rounds=2, t_rounds=2, decisions=decisions, drop=drop, taken=taken)
        return p, ols

    own = {}
    with torch.no_grad():
        _, free = oracle(None, own)
    for tag, got in runs.items():
        prob_dev = got['prob'].double()
        inside = (prob_dev > 0) & (prob_dev < 1)
        for k in range(2):
            assert not bool(((per_layer['relu'][k] != 0) & (drop[k] == 0)).any())
        flips = sum(int((((per_layer['relu'][k] > 0) != own['relu'][k]) & (drop[k] != 0)).sum()) for k in range(2))
        y = own['pre_clamp']
        flips += int((inside != ((y > 0) & (y < 1))).sum()) + int((torch.sign(prob_dev - label) != torch.sign(free['prob'] - label)).sum())
        _measure(test='train_step', ctype=ctype, path=tag, flips=flips, cap=_flip_cap(N))
        assert flips <= _flip_cap(N), (tag, flips)
        decisions = {'relu': [a > 0 for a in per_layer['relu']], 'inside': inside, 'sign': torch.sign(prob_dev - label)}
        p, ols = oracle(decisions)
        R.weighted_loss(ols, W).backward()
        for k in ('recon_loss', 'prob_loss', 'func_loss'):
            close(got['losses'][k], ols[k].detach().numpy(), rtol=1e-4, msg='%s %s' % (tag, k))
        worst = (0.0, '')
        for k, g in got['grads'].items():
            ref = p[k].grad
            if g is None:
                assert ref is None or float(ref.abs().max()) < 1e-5, k
                continue
            if ref is None:
                assert float(g.abs().max()) == 0.0, k
                continue
            g, ref = g.numpy(), ref.numpy()
            if 'attn_lin.weight' in k:
                g, ref = g[:, H:], ref[:, H:]
            scale = max(1e-6, float(np.abs(ref).max()))
            if k not in ('readout_prob.fc.0.bias', 'readout_prob.fc.4.bias'):       # mathematically zero: the floor below is theirs
                worst = max(worst, (float(np.abs(g - ref).max()) / scale, k))
            # 5e-6 floor: Linear biases in front of a BatchNorm have a mathematically zero gradient (noise on the device side)
            np.testing.assert_allclose(g, ref, rtol=2e-3, atol=grad_atol() * scale + 5e-6, err_msg='%s grad %s' % (tag, k))
        _measure(test='train_step', ctype=ctype, path=tag, worst_grad=worst[0], tensor=worst[1])
