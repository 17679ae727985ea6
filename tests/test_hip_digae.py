"""GPU tests of the DiGAE baseline (--model AE): the recorded reference run (tests/golden/g9_digae.npz) through the modules in both
precision modes, each entry of csrc/digcn_conv.hip on its own against the float64 restatement tests/digae_ref.py, one whole train
step against the oracle with the restatement as its structural encoder, and train.py --model AE through its three stages.
Nothing here reads the reference checkout.  The per-entry tests of those kernels (each output entry on its own scale, designed list
lengths) are in tests/test_hip_digae_entries.py; the one-bound-per-tensor entry tests below still cover the later grid passes at full
size (70,001 and 2^20 rows at every width), and with them stand the recorded reference run and the train step.

Bounds (the project's own): activations 2e-4 of scale (test_hip_encoder.py), losses 1e-4, gradients 1e-3 of each tensor's scale in
bf16x3 mode and 5e-4 in f32 mode.  The new kernels are exact fp32 in both modes; the modes differ in the Linear layers."""
import importlib
import os
import types

import numpy as np
import pytest
import torch

import digae_ref as R
from conftest import PKG_PARENT, load_golden
from test_digae_spec import CASES, build, fixture_case

pytestmark = pytest.mark.gpu
ACT_TOL, LOSS_TOL = 2e-4, 1e-4
NAN = float('nan')


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def grad_tol():
    from deepgate import ops
    return 5e-4 if ops.PRECISION == 'f32' else 1e-3


def err_of(a, ref, floor=0.0):
    """max |a - ref| over max(|ref|, floor), both moved to float64 on the host."""
    a, ref = a.detach().double().cpu(), (ref.detach() if torch.is_tensor(ref) else torch.as_tensor(np.asarray(ref))).double().cpu()
    return float((a - ref).abs().max()) / max(float(ref.abs().max()), floor, 1e-30)


# ------------------------------------------------------------------------------------------------
# the reference's recorded run
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['x3', 'f32'])
@pytest.mark.parametrize('p,path', [(p, path) for p in CASES for path in ('classes', 'rows') if (p, path) != ('float', 'classes')])
def test_fixture_case_hidden_embeddings_loss_and_every_gradient(p, path, precision, monkeypatch):
    """`classes`: the one-hot rows as integer x (the class-table first layer); `rows`: as float x [N, 6], zero-padded to the linear
    kernels' granule (the general first layer).  The float case has only the second form."""
    dev = _dev()
    import deepgate
    from deepgate import ops
    monkeypatch.setattr(ops, 'PRECISION', precision)
    z = load_golden('g9_digae')
    x, ei, neg, _ = fixture_case(z, p, torch.float32)
    enc = build(p)
    enc.load_state_dict({str(k): torch.from_numpy(z['%s_param_%s' % (p, k)]) for k in z[p + '_keys']}, strict=True)
    enc.to(dev)
    model = deepgate.digae_model.DirectedGAE(enc)
    ei, neg = ei.to(dev), neg.to(dev)
    x = x.to(dev)
    if path == 'classes':
        x = x.long()
    elif p == 'float':
        x.requires_grad_(True)
    plan = deepgate.GraphPlan(ei, x.shape[0])
    assert plan.heavy(True)[0] >= 1                       # the 70-consumer input takes the one-workgroup-per-list kernel
    if p != 'single':
        hs = enc.source_conv.conv1(x, ei, plan, False, relu=True)
        ht = enc.target_conv.conv1(x, ei, plan, True, relu=True)
        for name, h in (('hs', hs), ('ht', ht)):
            assert err_of(h, z['%s_%s' % (p, name)], 1.0) <= ACT_TOL, (name, err_of(h, z['%s_%s' % (p, name)], 1.0))
            # (no ReLU decision of the fixture is within 1e-4 of its layer's scale of zero: make_golden_digae.py)
            assert torch.equal(h.detach().cpu() > 0, torch.from_numpy(z['%s_%s' % (p, name)]) > 0), name
    s, t = model.encode(x, x, ei, plan=plan)
    for name, v in (('s', s), ('t', t)):
        assert err_of(v, z['%s_%s' % (p, name)], 1.0) <= ACT_TOL, (name, err_of(v, z['%s_%s' % (p, name)], 1.0))
    loss, pred_bin, gt_bin = model.recon_loss(s, t, ei, neg)
    ref_loss = float(z[p + '_loss'])
    assert abs(float(loss) - ref_loss) <= LOSS_TOL * max(1.0, abs(ref_loss)), (float(loss), ref_loss)
    assert int((pred_bin.cpu().numpy() != z[p + '_pred_bin']).sum()) <= 1          # a prediction flips only where sigma rounds across 0.5
    assert int(gt_bin.sum()) == ei.shape[1] and gt_bin.shape[0] == ei.shape[1] + neg.shape[1]
    loss.backward()
    for k, q in enc.named_parameters():
        e = err_of(q.grad, z['%s_grad_%s' % (p, k)])
        assert e <= grad_tol(), (k, e)
    if p == 'float':
        assert err_of(x.grad, z['float_dx']) <= grad_tol(), err_of(x.grad, z['float_dx'])
    auc, ap = model.test(s.detach(), t.detach(), ei, neg)
    assert 0.0 <= auc <= 1.0 and 0.0 < ap <= 1.0


# ------------------------------------------------------------------------------------------------
# the entries one by one
# ------------------------------------------------------------------------------------------------
def hub_node(n):
    """The hub sits at node 0, and at node 200,003 where there is one: in a later grid pass of the kernels."""
    return 200003 if n > 200003 else 0


def random_lists(n, rng, hub=0, mean_deg=2, empty_every=7):
    """edge_index [2, E] of a random directed multigraph on n nodes (duplicates and self edges allowed — the layer counts whatever the
    list holds): every `empty_every`-th node has no in-edges, node hub_node(n) receives `hub` extra edges and sends `hub` extra ones."""
    e = max(n * mean_deg, 1) if n > 1 else 2
    src, dst = rng.integers(0, n, e), rng.integers(0, n, e)
    keep = dst % empty_every != empty_every - 1
    src, dst = src[keep], dst[keep]
    if hub:
        other = rng.integers(0, n, 2 * hub)
        src = np.concatenate([src, other[:hub], np.full(hub, hub_node(n), dtype=src.dtype)])
        dst = np.concatenate([dst, np.full(hub, hub_node(n), dtype=dst.dtype), other[hub:]])
    return torch.from_numpy(np.stack([src, dst]).astype(np.int64))


def device_plan(ei, n, dev):
    from deepgate.graph_plan import GraphPlan
    plan = GraphPlan(ei.to(dev), n)
    plan._check_status()
    return plan


def call_scales(plan, reverse, alpha, beta, loops):
    from deepgate import _hip
    r = torch.full((plan.N,), NAN, device=plan.in_ptr.device)
    c = torch.full((plan.N,), NAN, device=plan.in_ptr.device)
    _hip.call('mgv_digcn_scales', plan.N, _hip.ptr(plan.csr(reverse)[0]), _hip.ptr(plan.csr(not reverse)[0]), alpha, beta, int(loops),
              _hip.ptr(r), _hip.ptr(c))
    return r, c


def call_gather(plan, reverse, y, outer, inner, mask, loops, relu, heavy=True):
    from deepgate import _hip
    p, i = plan.csr(reverse)
    hn, hnodes = plan.heavy(reverse) if heavy else (0, None)
    out = torch.full_like(y, NAN)
    _hip.call('mgv_digcn_gather', y.shape[1], plan.N, _hip.ptr(y), _hip.ptr(p), _hip.ptr(i), _hip.ptr(outer), _hip.ptr(inner), _hip.ptr(mask),
              int(loops), int(relu), hn, _hip.ptr(hnodes) if hn else None, _hip.ptr(out))
    return out


SIZES = [(1, 0), (2, 0), (63, 0), (64, 0), (65, 0), (700, 512), (700, 513), (9000, 5000), (70001, 0)]
# every size at every width (a workgroup holds 64, 32, 16 or 8 nodes at H = 16, 32, 64, 128: the block boundaries differ by width); 2^20 rows
# at H = 16 and 32 (several grid passes of every kernel, the hub in a later pass)
WIDTH_SIZES = [(H, n, hub) for H in (16, 32, 64, 128) for n, hub in SIZES] + [(16, 1 << 20, 0), (32, 1 << 20, 700)]


@pytest.mark.parametrize('n,hub', SIZES + [(1 << 20, 0)])
def test_scales_entry(n, hub):
    """r, c for every exponent pair out of {0, 0.5, 1} and two pairs of other exponents (the powf branch), with and without self loops,
    over both CSRs, against float64: 2 ulp of float32 for the exponents 0.5 and 1 (a correctly rounded division or square root and
    division), 16 ulp for a general exponent (the accuracy OpenCL asks of pow, which the device library's powf documents), exactly
    1 at an exponent of 0, exactly 0 (never inf) at a degree of 0."""
    dev = _dev()
    rng = np.random.default_rng(n + hub)
    ei = random_lists(n, rng, hub)
    plan = device_plan(ei, n, dev)
    pairs = [(a, b) for a in (0.0, 0.5, 1.0) for b in (0.0, 0.5, 1.0)] + [(0.3, 0.7), (1.5, 0.3)]
    if n > 100000:
        pairs = [(1.0, 0.0), (0.5, 0.5), (0.3, 0.7)]
    for loops in (True, False):
        for alpha, beta in pairs:
            for reverse in (False, True):
                e = R.flip(ei) if reverse else ei
                r, c = call_scales(plan, reverse, alpha, beta, loops)
                r2, c2 = call_scales(plan, reverse, alpha, beta, loops)
                assert torch.equal(r, r2) and torch.equal(c, c2)
                rr, cr = R.scales(e, n, alpha, beta, loops)
                for got, ref, a in ((r, rr, alpha), (c, cr, beta)):
                    got = got.double().cpu()
                    ulp = 2 if a in (0.0, 0.5, 1.0) else 16
                    assert bool(torch.isfinite(got).all())
                    assert float(((got - ref).abs() / ref.clamp_min(1e-30)).max()) <= ulp * 1.2e-7
                    assert bool((got[ref == 0] == 0).all())
                    if a == 0.0 and loops:
                        assert bool((got == 1).all())


@pytest.mark.parametrize('H,n,hub', WIDTH_SIZES)
def test_gather_entry_forward_and_pull(H, n, hub):
    """The scaled sum as the forward uses it (ReLU on and off) and as the backward does (opposite CSR, scales swapped, ReLU mask while
    gathering), with and without self loops, hubs on the one-workgroup-per-list kernel and on the plain one; output NaN-filled before
    the call; a repeated call is bit-identical."""
    dev = _dev()
    rng = np.random.default_rng(1000 * H + n + hub)
    ei = random_lists(n, rng, hub)
    plan = device_plan(ei, n, dev)
    if hub:
        assert plan.heavy(False)[0] >= 1 and plan.heavy(True)[0] >= 1
    g = torch.Generator().manual_seed(n)
    y = torch.randn(n, H, dtype=torch.float64, generator=g)
    z = torch.randn(n, H, dtype=torch.float64, generator=g)         # stands for a forward output: its sign pattern is the mask
    yd, zd = y.float().to(dev), z.float().to(dev)
    y, z = yd.double().cpu(), zd.double().cpu()
    for alpha, beta, loops in ((1.0, 0.0, True), (0.5, 0.5, True), (0.0, 1.0, False), (1.0, 1.0, False)):
        for reverse in (False, True):
            e = R.flip(ei) if reverse else ei
            r, c = call_scales(plan, reverse, alpha, beta, loops)
            ref = R.propagate(y, e, alpha, beta, loops)
            scale = max(1.0, float(ref.abs().max()))
            for heavy in ((True, False) if hub else (True,)):
                out = call_gather(plan, reverse, yd, r, c, None, loops, False, heavy)
                assert float((out.double().cpu() - ref).abs().max()) <= ACT_TOL * scale
                assert torch.equal(out, call_gather(plan, reverse, yd, r, c, None, loops, False, heavy))
                outr = call_gather(plan, reverse, yd, r, c, None, loops, True, heavy)
                assert float((outr.double().cpu() - torch.relu(ref)).abs().max()) <= ACT_TOL * scale
                # the pull: gradient of sum(out * w) w.r.t. y' where the layer is out = propagate(relu-masked y'), over the opposite CSR
                pull = call_gather(plan, not reverse, yd, c, r, zd, loops, False, heavy)
                yy = y.clone().requires_grad_(True)
                # d/dyy of <propagate(yy, e), y * [z > 0]> = c_j sum_{i: j in L(i)} r_i [z_i > 0] y_i
                (R.propagate(yy, e, alpha, beta, loops) * (y * (z > 0))).sum().backward()
                assert float((pull.double().cpu() - yy.grad).abs().max()) <= ACT_TOL * max(1.0, float(yy.grad.abs().max()))
                assert torch.equal(pull, call_gather(plan, not reverse, yd, c, r, zd, loops, False, heavy))


@pytest.mark.parametrize('H,n,hub', WIDTH_SIZES)
def test_class_entries(H, n, hub):
    """Class-table layer forward against propagate(T[cls]) and its backward dT against float64 autograd on the device's own ReLU mask;
    the number of ReLU decisions that differ from the oracle's is bounded separately."""
    dev = _dev()
    from deepgate import _hip
    rng = np.random.default_rng(77 * H + n + hub)
    ei = random_lists(n, rng, hub)
    plan = device_plan(ei, n, dev)
    g = torch.Generator().manual_seed(n + 1)
    for C, (alpha, beta, loops), reverse in ((6, (1.0, 0.0, True), False), (8, (0.5, 0.5, True), True), (1, (0.0, 1.0, False), False),
                                            (3, (1.0, 0.5, False), True)):
        cls = torch.from_numpy(rng.integers(0, C, n).astype(np.uint8))
        T = torch.randn(C, H, generator=g)
        dz = torch.randn(n, H, generator=g)
        e = R.flip(ei) if reverse else ei
        r, c = call_scales(plan, reverse, alpha, beta, loops)
        p, i = plan.csr(reverse)
        Td, cd, dzd = T.to(dev), cls.to(dev), dz.to(dev)

        def fwd(relu):
            out = torch.full((n, H), NAN, device=dev)
            _hip.call('mgv_digcn_class_fwd', H, n, _hip.ptr(cd), _hip.ptr(Td), C, _hip.ptr(p), _hip.ptr(i), _hip.ptr(r), _hip.ptr(c), int(loops),
                      int(relu), _hip.ptr(out))
            return out

        def bwd(zmask):
            dT = torch.zeros(C, H, device=dev)
            ws = torch.full((max(_hip.call_value('mgv_digcn_class_bwd_ws_floats', H, n), 1),), NAN, device=dev)
            _hip.call('mgv_digcn_class_bwd', H, n, _hip.ptr(cd), C, _hip.ptr(p), _hip.ptr(i), _hip.ptr(r), _hip.ptr(c), int(loops), _hip.ptr(zmask),
                      _hip.ptr(dzd), _hip.ptr(dT), _hip.ptr(ws), ws.numel())
            return dT

        T64 = T.double().requires_grad_(True)
        pre = R.propagate(T64[cls.long()], e, alpha, beta, loops)
        scale = max(1.0, float(pre.abs().max()))
        z0, z1 = fwd(False), fwd(True)
        assert float((z0.double().cpu() - pre.detach()).abs().max()) <= ACT_TOL * scale
        assert float((z1.double().cpu() - torch.relu(pre.detach())).abs().max()) <= ACT_TOL * scale
        assert torch.equal(z1, fwd(True))
        mask = (z1 > 0).cpu()
        differ = int((mask != (pre.detach() > 0)).sum())
        assert differ <= max(4, int(1e-4 * mask.numel())), differ
        for zmask, m in ((None, None), (z1, mask)):
            T64.grad = None
            ((pre if m is None else pre * m) * dz.double()).sum().backward(retain_graph=True)
            dT = bwd(zmask)
            assert err_of(dT, T64.grad) <= 5e-4, err_of(dT, T64.grad)
            assert torch.equal(dT, bwd(zmask))


# ------------------------------------------------------------------------------------------------
# the encoder at a size past the grid cap, both modes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['x3', 'f32'])
def test_encoder_past_the_grid_cap_with_a_hub(precision, monkeypatch):
    """DirectedGCNConvEncoder 6 -> 64 -> 64 on 70,001 nodes (more than one grid pass of the scaled-sum and class kernels at this width; the scales launch and the
    narrower widths take their later passes in the entry tests at 2^20 nodes), a 5,000-entry hub in both
    directions, class-table first layer: hidden, s, t and every parameter gradient against the float64 restatement evaluated on the
    device's own ReLU mask; the decisions that differ from the restatement's own are counted separately.  Two backward passes give
    bit-identical gradients in bf16x3 mode (the fp32 weight-gradient kernel of f32 mode adds with atomics, as before)."""
    dev = _dev()
    from deepgate import ops
    from deepgate.graph_plan import GraphPlan
    monkeypatch.setattr(ops, 'PRECISION', precision)
    n = 70001
    rng = np.random.default_rng(5)
    ei = random_lists(n, rng, 5000)
    cls = torch.from_numpy(rng.integers(0, 6, n).astype(np.uint8))
    enc = build('a1b0')
    p64 = {k: v.detach().double().clone().requires_grad_(True) for k, v in enc.state_dict().items()}
    enc.to(dev)
    plan = GraphPlan(ei.to(dev), n)
    rows = torch.eye(6, device=dev)
    g = torch.Generator().manual_seed(9)
    ws, wt = torch.randn(n, 64, generator=g), torch.randn(n, 64, generator=g)

    def step():
        enc.zero_grad()
        hs = enc.source_conv.conv1(None, None, plan, False, (rows, cls.to(dev)), relu=True)
        ht = enc.target_conv.conv1(None, None, plan, True, (rows, cls.to(dev)), relu=True)
        s, t = enc(None, None, None, plan=plan, classes=(rows, cls.to(dev)))
        ((s * ws.to(dev)).sum() + (t * wt.to(dev)).sum()).backward()
        return hs.detach(), ht.detach(), s.detach(), t.detach(), {k: q.grad.clone() for k, q in enc.named_parameters()}

    hs, ht, s, t, grads = step()
    x = torch.eye(6, dtype=torch.float64)[cls.long()]
    _, _, hs0, ht0 = R.encoder(p64, '', x, x, ei)
    differ = int(((hs.cpu() > 0) != (hs0 > 0)).sum()) + int(((ht.cpu() > 0) != (ht0 > 0)).sum())
    assert differ <= max(4, int(1e-4 * 2 * hs.numel())), differ
    masks = ((hs > 0).cpu(), (ht > 0).cpu())
    s64, t64, hs64, ht64 = R.encoder(p64, '', x, x, ei, relu_mask=masks)
    ((s64 * ws.double()).sum() + (t64 * wt.double()).sum()).backward()
    for name, a, b in (('hs', hs, hs64), ('ht', ht, ht64), ('s', s, s64), ('t', t, t64)):
        assert err_of(a, b, 1.0) <= ACT_TOL, (name, err_of(a, b, 1.0))
    for k, q in grads.items():
        assert err_of(q, p64[k].grad) <= grad_tol(), (k, err_of(q, p64[k].grad))
    if precision == 'x3':
        again = step()[4]
        assert all(torch.equal(grads[k], again[k]) for k in grads)


# ------------------------------------------------------------------------------------------------
# one whole train step with the baseline encoder
# ------------------------------------------------------------------------------------------------
def _ae_model(dev, seed):
    import deepgate
    torch.manual_seed(seed)
    enc = deepgate.digae_layer.DirectedGCNConvEncoder(6, 64, 64, 1.0, 0.0, True, False)
    model = deepgate.dg_ae_model_aig.Model(struct_encoder=enc, dim_hidden=64)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return model


@pytest.mark.parametrize('size', ['small', 'baseline_graph'])
def test_train_step_with_the_baseline_encoder_matches_the_oracle(size, monkeypatch):
    """Trainer.run_batch, backward and the Adam step with DirectedGCNConvEncoder as the AIG Model's structural encoder against
    oracle/ref_cpu.run_batch, whose struct_encoder is replaced (in this test only) by the restatement: the three losses, every
    parameter gradient, the parameters after one step.  `small`: four 256-node graphs; `baseline_graph`: one 65,536-node graph."""
    dev = _dev()
    import deepgate
    from deepgate import synthetic as syn
    from oracle import ref_cpu as O
    monkeypatch.setattr(O, 'struct_encoder', lambda p, prefix, x, ei, s_rounds, t_rounds, layernorm=True:
                        R.encoder(p, prefix + '.', x.to(p[prefix + '.source_conv.conv1.lin.weight'].dtype), x.to(p[prefix + '.source_conv.conv1.lin.weight'].dtype), ei)[:2])
    if size == 'small':
        arrays = syn.collate([syn.make_graph('aig', 256, 8, 900 + i, n_inputs=16) for i in range(4)])
    else:
        arrays = syn.make_batch(2, batch=1)
    model = _ae_model(dev, 11)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    model.to(dev).train()
    weights = [1.0, 4.0, 4.0]
    tr = deepgate.Trainer(types.SimpleNamespace(model='AE'), model, training_id='ae', save_dir='/tmp/mgv_test_exp', lr=1e-4,
                          rc_prob_func_weight=weights, device='cuda:0', batch_size=1, distributed=False)
    assert tr._encoder_half_rounds() == []
    batch = deepgate.CircuitBatch.from_arrays(arrays, device=dev)
    tr.optimizer.zero_grad()
    ls = tr.run_batch(batch, want_pred=False)
    tr.weighted_loss(ls).backward()
    torch.cuda.synchronize()
    grads = {k: q.grad.detach().cpu().clone() for k, q in model.named_parameters() if q.grad is not None}
    tr.optimizer.step()
    after = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}

    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    p = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and 'running_' not in k else v.clone()) for k, v in sd.items()}
    bn = {k: v.clone() for k, v in p.items() if 'running_' in k}
    ob = O.batch_from_arrays(lambda k: arrays[k])
    plan = O.LevelPlan('aig', ob['edge_index'], ob['gate'], ob['forward_level'])
    ols = O.run_batch(p, 'aig', ob, training=True, bn_state=bn, p_drop=0.0, plan=plan, fast=True)
    O.weighted_loss(ols, weights).backward()
    for k in ('recon_loss', 'prob_loss', 'func_loss'):
        a, b = float(ls[k].detach()), float(ols[k].detach())
        assert abs(a - b) <= LOSS_TOL * max(1.0, abs(b)), (k, a, b)
    dead = ('msg_q.', 'msg_k.bias', 'attn_lin.bias', 'func.weight_hh_l0')
    for k, q in model.named_parameters():
        ref = p[k].grad
        ref = (torch.zeros_like(p[k]) if ref is None else ref).numpy()
        if k not in grads:
            assert any(d in k for d in dead) or 'attn_lin.weight' in k, k
            assert float(np.abs(ref).max()) < 1e-5, (k, float(np.abs(ref).max()))
            continue
        gk = grads[k].numpy()
        if 'attn_lin.weight' in k:
            H = ref.shape[1] // 2
            gk, ref = gk[:, H:], ref[:, H:]
        scale = float(np.abs(ref).max())
        if k in ('readout_prob.fc.0.bias', 'readout_prob.fc.4.bias'):
            # a Linear bias in front of BatchNorm: a mathematically zero gradient, priced against the layer's weight gradient
            # (as in test_hip_fullsize.py)
            scale = float(p[k.replace('bias', 'weight')].grad.abs().max())
        if scale < 1e-7:
            assert float(np.abs(gk).max()) < 1e-6, k
            continue
        e = float(np.abs(gk - ref).max()) / scale
        if 'struct_encoder' in k:
            print('   %-48s %.2e of scale %.2e' % (k, e, scale))
        assert e <= grad_tol(), (k, e, scale)
    opt = torch.optim.Adam(O.trainable(p), lr=1e-4)
    opt.step()
    for k, q in model.named_parameters():
        if size == 'baseline_graph' and k in ('readout_prob.fc.0.bias', 'readout_prob.fc.4.bias'):
            continue             # mathematically zero gradients (a bias in front of a BatchNorm): over 65,536 rows either side's rounding noise passes the 1e-5 `live` threshold and Adam turns it into full steps; the small batch keeps them, as test_hip_model.py does
        if k in grads and p[k].grad is not None:
            live = (p[k].grad.abs() > 1e-5).numpy()
            np.testing.assert_allclose(after[k].numpy()[live], p[k].detach().numpy()[live], rtol=1e-5, atol=3e-6, err_msg='adam ' + k)


def test_train_entry_with_model_ae_and_checkpoint_reload(tmp_path, monkeypatch):
    """`python train.py --model AE --type aig --synthetic ...` through its three stages; the checkpoint holds the baseline encoder's
    eight tensors, loads strictly into a fresh model and gives the same embeddings."""
    dev = _dev()
    import deepgate
    from deepgate import synthetic as syn
    monkeypatch.syspath_prepend(PKG_PARENT)
    train = importlib.import_module('train')
    train.main(['--exp_id', 'ae', '--model', 'AE', '--type', 'aig', '--batch_size', '2', '--synthetic', '6', '--synthetic_nodes', '256',
                '--synthetic_levels', '8', '--stage_epochs', '1', '1', '1', '--save_dir', str(tmp_path)])
    cp = torch.load(tmp_path / 'ae' / 'stage_3.pth', map_location='cpu')
    assert cp['epoch'] == 3 and all(torch.isfinite(v).all() for v in cp['state_dict'].values() if v.is_floating_point())
    enc_keys = [k for k in cp['state_dict'] if k.startswith('struct_encoder.')]
    assert enc_keys == ['struct_encoder.' + k for k in build('a1b0').state_dict().keys()]
    first = torch.load(tmp_path / 'ae' / 'stage_1.pth', map_location='cpu')
    assert any(not torch.equal(first['state_dict'][k], cp['state_dict'][k]) for k in enc_keys)       # the encoder trains
    log = [f for f in os.listdir(tmp_path / 'ae') if f.startswith('log-')]
    text = open(tmp_path / 'ae' / log[0]).read()
    assert text.count('train| Epoch') == 3 and 'nan' not in text.lower()
    models = []
    for _ in range(2):
        m = deepgate.dg_ae_model_aig.Model(struct_encoder=build('a1b0'), dim_hidden=64)
        m.load_state_dict(cp['state_dict'], strict=True)
        models.append(m.to(dev).eval())
    batch = deepgate.CircuitBatch.from_arrays(syn.collate([syn.make_graph('aig', 256, 8, 100, n_inputs=16)]), device=dev)
    with torch.no_grad():
        a, b = models[0](batch), models[1](batch)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and bool(torch.isfinite(a[1]).all())
