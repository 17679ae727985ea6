"""GPU parity of the full DG_AE path through the reference's operator surface (Model / Trainer):
outputs, losses, gradients of every parameter and one Adam step against the golden vectors the
reference produced, plus per-operator fixtures.  fp32 on both sides, different summation order:
tolerances stated per assert (2e-4 relative to the tensor's scale unless noted)."""
import types

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
TYPES = ['aig', 'mig', 'xag', 'xmg']


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def load(name):
    return load_golden(name)


def grad_atol():
    """Gradient tolerance relative to the tensor's largest entry: 1e-4 for the exact-fp32 kernels,
    1e-3 for the default bf16x3 split-precision kernels (~1e-5 per product, chained through 16 half
    rounds forward and backward)."""
    from deepgate import ops
    return 1e-4 if ops.PRECISION == "f32" else 1e-3


def close(a, b, rtol=2e-4, atol=2e-5, msg=''):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    scale = max(1e-6, float(np.abs(b).max()))
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol * scale + 1e-7, err_msg=msg)


def build(z, dev):
    import deepgate
    ctype, H, R = str(z['meta_type']), int(z['meta_H']), int(z['meta_R'])
    enc = deepgate.digae_layer.DirectMultiGCNEncoder(dim_feature=6, dim_hidden=H, s_rounds=R, t_rounds=R, layernorm=True)
    mod = {'aig': deepgate.dg_ae_model_aig, 'mig': deepgate.dg_ae_model_mig, 'xag': deepgate.dg_ae_model_xag,
           'xmg': deepgate.dg_ae_model_xmg}[ctype]
    model = mod.Model(struct_encoder=enc, dim_hidden=H, enable_encode=True, enable_reverse=True)
    sd = {k[len('param_'):]: torch.tensor(z[k]) for k in z.files if k.startswith('param_')}
    model.load_state_dict(sd, strict=True)
    model.to(dev)
    batch = deepgate.CircuitBatch.from_arrays({k[3:]: z[k] for k in z.files if k.startswith('in_')}, device=dev)
    return model, batch


@pytest.mark.parametrize('name', ['g1_' + t for t in TYPES] + ['g2_aig', 'g2_xmg'])
def test_eval_forward_matches_reference(name):
    dev = _dev()
    z = load(name)
    model, batch = build(z, dev)
    model.eval()
    with torch.no_grad():
        hs, hf = model(batch)
        prob = model.pred_prob(hf)
        rl, pred_bin, gt_bin = model.recon_loss(hs, batch.edge_index, batch.neg_edge_index)
    close(hs, z['eval_hs'], msg='hs')
    close(hf, z['eval_hf'], msg='hf')
    close(prob, z['eval_prob'], msg='prob')
    close(rl, z['eval_recon'], rtol=1e-4, msg='recon loss')          # north_star: loss match 1e-4
    # a prediction can flip only where sigma is within rounding of 0.5
    flips = int((pred_bin.cpu().numpy() != z['eval_pred_bin']).sum())
    assert flips <= 1, flips
    assert np.array_equal(gt_bin.cpu().numpy(), z['eval_gt_bin'])
    cnt = model.last_confusion.cpu().numpy()
    pb, gb = z['eval_pred_bin'], z['eval_gt_bin']
    ref = [int(((pb == 1) & (gb == 1)).sum()), int(((pb == 1) & (gb == 0)).sum()),
           int(((pb == 0) & (gb == 0)).sum()), int(((pb == 0) & (gb == 1)).sum())]
    assert np.abs(cnt - np.array(ref)).sum() <= 2 * flips


@pytest.mark.parametrize('name', ['g1_' + t for t in TYPES] + ['g2_aig', 'g2_xmg'])
def test_train_step_losses_grads_adam_match_reference(name):
    dev = _dev()
    import deepgate
    z = load(name)
    model, batch = build(z, dev)
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    args = types.SimpleNamespace(model='DG_AE')
    tr = deepgate.Trainer(args, model, training_id='t', save_dir='/tmp/mgv_test_exp', lr=float(z['meta_lr']),
                          rc_prob_func_weight=[float(v) for v in z['meta_weights']], device='cuda:0', batch_size=1,
                          distributed=False)
    tr.optimizer.zero_grad()
    ls = tr.run_batch(batch)
    loss = tr.weighted_loss(ls)
    close(ls['recon_loss'], z['train_recon'], rtol=1e-4, msg='recon')
    close(ls['prob_loss'], z['train_prob_loss'], rtol=1e-4, msg='prob loss')
    close(ls['func_loss'], z['train_func_loss'], rtol=1e-4, msg='func loss')
    close(loss, z['train_loss'], rtol=1e-4, msg='total')
    assert abs(int(ls['pred_bin'].sum()) - int(z['train_pred_bin_sum'])) <= 1
    assert int(ls['gt_bin'].sum()) == int(z['train_gt_bin_sum'])
    loss.backward()
    dead = ('msg_q.', 'msg_k.bias', 'attn_lin.bias', 'func.weight_hh_l0')
    for k, p in model.named_parameters():
        ref = z['grad_' + k]
        if p.grad is None:
            # branches that cancel inside the per-destination softmax / multiply a zero state: the
            # reference's gradient there is rounding noise
            assert any(d in k for d in dead) or 'attn_lin.weight' in k, k
            assert float(np.abs(ref).max()) < 1e-5, (k, float(np.abs(ref).max()))
            continue
        g = p.grad.detach().cpu().numpy()
        if 'attn_lin.weight' in k:          # q half is dead, k half is live
            H = ref.shape[1] // 2
            assert float(np.abs(ref[:, :H]).max()) < 1e-5
            g, ref = g[:, H:], ref[:, H:]
        scale = max(1e-6, float(np.abs(ref).max()))
        if k in ('readout_prob.fc.0.bias', 'readout_prob.fc.4.bias'):
            # a Linear bias in front of BatchNorm (mlp.py:29-32): the gradient is mathematically zero, the reference's and ours are the
            # rounding noise of a column sum (~1e-6, order-dependent); priced against the layer's weight gradient
            scale = max(scale, float(np.abs(z['grad_' + k.replace('bias', 'weight')]).max()))
        np.testing.assert_allclose(g, ref, rtol=1e-3, atol=grad_atol() * scale + 1e-6, err_msg='grad ' + k)
    if 'after_hs_linear.weight' in z.files:
        tr.optimizer.step()
        sd = model.state_dict()
        for k, p in model.named_parameters():
            live = np.abs(z['grad_' + k]) > 1e-5
            np.testing.assert_allclose(sd[k].cpu().numpy()[live], z['after_' + k][live], rtol=1e-5, atol=3e-6, err_msg='adam ' + k)
        for k in sd:
            if 'running_' in k:
                close(sd[k], z['after_' + k], rtol=1e-4, atol=1e-5, msg=k)
            if 'num_batches_tracked' in k:
                assert int(sd[k]) == int(z['after_' + k])


def test_functional_level_op_vs_reference_fixture():
    """One level of TFMlpAggr + GRU (h0 = 0) through the C ABI, fan-in 1..5."""
    dev = _dev()
    from deepgate import ops, _hip
    from deepgate.graph_plan import GraphPlan
    from deepgate.arch.tfmlp import TFMlpAggr
    z = load('g3_ops')
    H = 64
    aggr = TFMlpAggr(2 * H, H)
    aggr.load_state_dict({k[len('lvl_aggr_'):]: torch.tensor(z[k]) for k in z.files if k.startswith('lvl_aggr_')})
    gru = torch.nn.GRU(H, H)
    gru.load_state_dict({k[len('lvl_gru_'):]: torch.tensor(z[k]) for k in z.files if k.startswith('lvl_gru_')})
    aggr.to(dev); gru.to(dev)
    ei = torch.tensor(z['lvl_edge_index'], device=dev)
    nodes = z['lvl_nodes']
    N = 40
    gate = torch.zeros(N, 1); gate[nodes] = 1
    level = torch.zeros(N, dtype=torch.long); level[nodes] = 1
    plan = GraphPlan(ei, N).set_levels(gate, level, [1])
    ns = torch.tensor(z['lvl_node_state'], device=dev)
    hs = ns[:, :H].contiguous()
    hf = ns[:, H:].contiguous()          # sources carry a non-zero functional state
    comp = aggr.composed(gru)
    par = [t.detach().unsqueeze(0).contiguous() for t in comp]
    ltp = (_hip.ctypes.c_int32 * len(plan.level_tile_ptr))(*plan.level_tile_ptr)
    P = _hip.ptr
    _hip.call('mgv_func_sweep_fwd', H, N, 1, plan.num_levels, ltp, P(plan.order), P(plan.tile_start), P(plan.tile_count),
              P(plan.tile_slot), P(plan.in_ptr), P(plan.in_src), P(hs), P(hf), *[P(t) for t in par], None, None)
    close(hf[torch.tensor(nodes, device=dev)], z['lvl0_hnew'], msg='hf of the level')
    # backward: upstream gradient on the level's rows
    ghf = torch.zeros(N, H, device=dev)
    ghf[torch.tensor(nodes, device=dev)] = torch.tensor(z['lvl_up'], device=dev)
    ghs = torch.zeros(N, H, device=dev)
    dzb = torch.zeros(N, 2 * H, device=dev)
    alpha = torch.zeros(ei.shape[1], device=dev); dsc = torch.zeros(ei.shape[1], device=dev)
    grads = [torch.zeros_like(t) for t in par]
    WvcT = par[1].transpose(1, 2).contiguous()
    _hip.call('mgv_func_sweep_bwd', H, N, 1, plan.num_levels, ltp, P(plan.order), P(plan.tile_start), P(plan.tile_count),
              P(plan.tile_slot), P(plan.in_ptr), P(plan.in_src), P(plan.out_ptr), P(plan.out_dst), P(plan.out_slot),
              P(plan.gslot), P(hs), P(hf), P(par[0]), P(par[1]), P(WvcT), P(par[2]), P(par[3]), P(par[4]), P(ghf), P(ghs),
              P(dzb), P(alpha), P(dsc), *[P(g) for g in grads], None, None, None, None)
    close(ghs, z['lvl0_grad_node_state'][:, :H], msg='grad hs')
    # the gradient wrt the sources' hf is what their own tiles would pull: rebuild it on the host
    al, ds = alpha.cpu().numpy(), dsc.cpu().numpy()
    gsrc = np.zeros((N, H), dtype=np.float64)
    u = par[0][0].cpu().numpy()
    in_src, in_dst = plan.in_src.cpu().numpy(), plan.in_dst.cpu().numpy()
    act = plan.gslot.cpu().numpy() != 255
    dz = dzb.cpu().numpy()
    for e in range(len(in_src)):
        if act[in_dst[e]]:
            gsrc[in_src[e]] += al[e] * dz[in_dst[e], H:] + ds[e] * u[H:]
    close(gsrc.astype(np.float32), z['lvl0_grad_node_state'][:, H:], msg='grad hf of sources')
    torch.autograd.backward(list(comp), [g[0] for g in grads])
    for k, p in list(aggr.named_parameters()) + list(gru.named_parameters()):
        pre = 'lvl0_grad_aggr_' if any(p is q for q in aggr.parameters()) else 'lvl0_grad_gru_'
        ref = z[pre + k]
        if p.grad is None:
            assert float(np.abs(ref).max()) < 1e-5, k
            continue
        g = p.grad.cpu().numpy()
        if k == 'attn_lin.weight':
            g, ref = g[:, H:], ref[:, H:]
        scale = max(1e-6, float(np.abs(ref).max()))
        np.testing.assert_allclose(g, ref, rtol=1e-3, atol=1e-4 * scale + 1e-6, err_msg=k)


def test_readout_mlp_batchnorm_train_mode():
    dev = _dev()
    from deepgate import ops
    from deepgate.arch.mlp import MLP
    z = load('g3_ops')
    mlp = MLP(64, 32, 1, num_layer=3, p_drop=0.2, norm_layer='batchnorm', act_layer='relu')
    sd = {k[len('mlp_param_'):]: torch.tensor(z[k]) for k in z.files if k.startswith('mlp_param_')}
    for b in (1, 5):      # the fixture holds the buffers AFTER the training-mode forward
        sd['fc.%d.running_mean' % b] = torch.zeros(32); sd['fc.%d.running_var' % b] = torch.ones(32)
        sd['fc.%d.num_batches_tracked' % b] = torch.tensor(0)
    mlp.load_state_dict(sd)
    for m in mlp.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    mlp.to(dev).train()
    x = torch.tensor(z['mlp_in'], device=dev, requires_grad=True)
    prob = mlp(x, clamp01=True)
    close(prob, z['mlp_prob'], msg='prob')
    l1 = ops.l1_loss(prob, torch.tensor(z['mlp_target'], device=dev))
    close(l1, z['mlp_l1'], rtol=1e-5, msg='l1')
    l1.backward()
    close(x.grad, z['mlp_grad_in'], rtol=1e-3, atol=1e-4, msg='grad in')
    for k, p in mlp.named_parameters():
        ref = z['mlp_grad_' + k]
        scale = max(1e-6, float(np.abs(ref).max()))
        np.testing.assert_allclose(p.grad.cpu().numpy(), ref, rtol=1e-3, atol=1e-4 * scale + 1e-6, err_msg=k)
    sd2 = mlp.state_dict()
    close(sd2['fc.1.running_mean'], z['mlp_after_running_mean1'], msg='rm1')
    close(sd2['fc.1.running_var'], z['mlp_after_running_var1'], msg='rv1')
    close(sd2['fc.5.running_mean'], z['mlp_after_running_mean5'], msg='rm5')
    close(sd2['fc.5.running_var'], z['mlp_after_running_var5'], msg='rv5')


def test_dropout_mask_statistics_and_backward_consistency():
    dev = _dev()
    from deepgate import ops
    N, C = 20000, 32
    y = torch.randn(N, C, device=dev, requires_grad=True)
    g, b = torch.ones(C, device=dev), torch.full((C,), 5.0, device=dev)     # bn_out > 0 everywhere
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    a = ops.BnReluDropFn.apply(y, g, b, rm, rv, True, 0.2, 1234, 0.1, 1e-5)
    kept = (a != 0).float().mean().item()
    assert abs(kept - 0.8) < 0.01, kept
    a2 = ops.BnReluDropFn.apply(y, g, b, rm.clone(), rv.clone(), True, 0.2, 1234, 0.1, 1e-5)
    assert torch.equal(a, a2)                       # same seed, same mask
    a.sum().backward(retain_graph=True)             # gradient flows only through kept elements
    # ... which the backward has to find again from (seed, element): with bn_out > 0 everywhere, dz = upstream x factor, factor 0
    # where the forward dropped and 1/(1-p) where it kept, and dy is the BatchNorm backward of that dz.  Held to float64 autograd
    # through batch_norm x the forward's own factors (1e-5 of scale: an element-wise fp32 kernel with double column sums).
    fac = (a.detach() != 0).double().cpu() / (1.0 - float(np.float32(0.2)))
    y64 = y.detach().cpu().double().requires_grad_(True)
    g64, b64 = g.cpu().double().requires_grad_(True), b.cpu().double().requires_grad_(True)
    (torch.nn.functional.batch_norm(y64, None, None, g64, b64, training=True, eps=1e-5) * fac).sum().backward()
    err = float((y.grad.cpu().double() - y64.grad).abs().max()) / float(y64.grad.abs().max())
    assert err <= 1e-5, err
    # one unit at a time: a dropped unit passes nothing back, a kept one 1/(1-p) times the BatchNorm backward of the one-hot
    bn0 = torch.nn.functional.batch_norm(y64, None, None, g64, b64, training=True, eps=1e-5)
    keep = a.detach() != 0
    for want_kept in (False, True):
        i, c = [int(v) for v in torch.nonzero(keep == want_kept)[1234].tolist()]
        up = torch.zeros(N, C)
        up[i, c] = 1.0
        dy, = torch.autograd.grad(a, y, up.to(dev), retain_graph=True)
        if not want_kept:
            assert float(dy.abs().max()) == 0.0
            continue
        ref, = torch.autograd.grad(bn0, y64, up.double(), retain_graph=True)
        ref = ref / (1.0 - float(np.float32(0.2)))
        assert float((dy.cpu().double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


def test_func_loss_decoder_and_confusion_vs_reference_fixture():
    dev = _dev()
    from deepgate import ops
    from deepgate.digae_layer import DirectedInnerProductDecoder
    z = load('g3_ops')
    hf = torch.tensor(z['fl_hf'], device=dev, requires_grad=True)
    fl = ops.func_loss(hf, torch.tensor(z['fl_pairs'], device=dev), torch.tensor(z['fl_tt'], device=dev))
    close(fl, z['fl_loss'], rtol=1e-5, msg='func loss')
    fl.backward()
    close(hf.grad, z['fl_grad_hf'], rtol=1e-3, atol=1e-4, msg='func loss grad')
    # the pull-based backward (pairs grouped per node by csrc/plan_build.hip; no atomics, no zero fill) against the same fixture;
    # the fixture's random pairs contain repeated nodes and may contain a == b
    holder = types.SimpleNamespace()
    hf2 = torch.tensor(z['fl_hf'], device=dev, requires_grad=True)
    fl2 = ops.func_loss(hf2, torch.tensor(z['fl_pairs'], device=dev), torch.tensor(z['fl_tt'], device=dev), cache=holder)
    assert hasattr(holder, '_mgv_pair_lists') and float(fl2) == float(fl)
    fl2.backward()
    close(hf2.grad, z['fl_grad_hf'], rtol=1e-3, atol=1e-4, msg='func loss grad (pull)')
    assert float((hf2.grad - hf.grad).abs().max()) <= 1e-6 * float(hf.grad.abs().max()) + 1e-9
    hf3 = hf2.detach().clone().requires_grad_(True)
    ops.func_loss(hf3, torch.tensor(z['fl_pairs'], device=dev), torch.tensor(z['fl_tt'], device=dev), cache=holder).backward()
    assert torch.equal(hf3.grad, hf2.grad)                 # bit-reproducible
    dec = DirectedInnerProductDecoder()
    s, t = torch.tensor(z['dec_s'], device=dev), torch.tensor(z['dec_t'], device=dev)
    ei = torch.tensor(z['dec_edge_index'], device=dev)
    close(dec(s, t, ei, sigmoid=True), z['dec_sig'], rtol=1e-5, atol=1e-6, msg='decoder sigmoid')
    close(dec(s, t, ei, sigmoid=False), z['dec_raw'], rtol=1e-5, atol=1e-6, msg='decoder raw')
    # decoder autograd against torch on the host
    s1, t1 = s.clone().requires_grad_(True), t.clone().requires_grad_(True)
    w = torch.randn(ei.shape[1], device=dev)
    (dec(s1, t1, ei) * w).sum().backward()
    sc, tc = s.cpu().requires_grad_(True), t.cpu().requires_grad_(True)
    (torch.sigmoid((sc[ei[0].cpu()] * tc[ei[1].cpu()]).sum(1)) * w.cpu()).sum().backward()
    close(s1.grad, sc.grad, rtol=1e-4, atol=1e-5, msg='decoder ds')
    close(t1.grad, tc.grad, rtol=1e-4, atol=1e-5, msg='decoder dt')
    pred = torch.tensor([1, 0, 1, 1, 0, 0, 1], dtype=torch.int32, device=dev)
    gt = torch.tensor([1, 1, 0, 1, 0, 1, 0], dtype=torch.int32, device=dev)
    assert ops.confusion_counts(pred, gt).tolist() == [2, 2, 1, 2]      # TP FP TN FN


def test_vae_sampler_and_kl_vs_reference_fixture():
    dev = _dev()
    import deepgate
    z = load('g4_vae')
    H = 64
    enc = deepgate.digae_layer.DirectMultiGCNEncoder(dim_hidden=H, dim_feature=6, s_rounds=1, t_rounds=1, layernorm=True)
    vae = deepgate.digvae_model.DirectedGVAE(enc, H)
    vae.load_state_dict({k[len('param_'):]: torch.tensor(z[k]) for k in z.files if k.startswith('param_')}, strict=False)
    vae.to(dev)
    s = torch.tensor(z['s'], device=dev, requires_grad=True)
    t = torch.tensor(z['t'], device=dev, requires_grad=True)
    zs, zt = vae.sample(s, t, torch.tensor(z['eps_s'], device=dev), torch.tensor(z['eps_t'], device=dev))
    close(zs, z['sample_s'], msg='sample_s')
    close(zt, z['sample_t'], msg='sample_t')
    skl, tkl = vae.kl_loss()
    close(skl, z['s_kl'], rtol=1e-5, msg='s_kl')
    close(tkl, z['t_kl'], rtol=1e-5, msg='t_kl')
    ((zs * torch.tensor(z['up_s'], device=dev)).sum() + (zt * torch.tensor(z['up_t'], device=dev)).sum()
     + float(z['kl_weight']) * (skl + tkl)).backward()
    close(s.grad, z['grad_s'], rtol=1e-3, atol=1e-4, msg='grad s')
    close(t.grad, z['grad_t'], rtol=1e-3, atol=1e-4, msg='grad t')
    for k, p in vae.named_parameters():
        if k.startswith('fc_'):
            close(p.grad, z['grad_' + k], rtol=1e-3, atol=1e-4, msg=k)
    # the built-in generator: unit-variance, zero-mean noise, reproducible per seed
    z1, _ = vae.sample(s.detach(), t.detach(), seed=7)
    z2, _ = vae.sample(s.detach(), t.detach(), seed=7)
    assert torch.equal(z1, z2)
    eps = (z1 - vae.s_mu) / torch.exp(vae.s_logstd)
    assert abs(float(eps.mean())) < 0.05 and abs(float(eps.std()) - 1.0) < 0.05


@pytest.mark.parametrize('H,ctype', [(32, 'aig'), (32, 'xmg'), (16, 'mig'), (64, 'xag'), (64, 'mig')])
def test_other_hidden_widths_against_the_oracle(H, ctype):
    """dim_hidden 32 (bf16x3 kernels, split-K wgrad layout) and 16 (exact-fp32 kernels): no reference
    fixture exists at these widths, so the pinned oracle is the checker: same random parameters, same
    synthetic graphs, outputs + losses + every parameter gradient."""
    dev = _dev()
    import deepgate
    from deepgate import synthetic as syn
    from oracle import ref_cpu as R
    torch.manual_seed(5)
    enc = deepgate.digae_layer.DirectMultiGCNEncoder(dim_feature=6, dim_hidden=H, s_rounds=2, t_rounds=2, layernorm=True)
    mod = getattr(deepgate, 'dg_ae_model_' + ctype)
    model = mod.Model(struct_encoder=enc, dim_hidden=H)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, (torch.nn.LayerNorm, torch.nn.BatchNorm1d)):
                m.weight.add_(0.2 * torch.randn_like(m.weight)); m.bias.add_(0.2 * torch.randn_like(m.bias))
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model.to(dev).train()
    arrays = syn.collate([syn.make_graph(ctype, 150, 6, 600 + i, n_inputs=12) for i in range(3)])
    batch = deepgate.CircuitBatch.from_arrays(arrays, device=dev)
    tr = deepgate.Trainer(types.SimpleNamespace(model='DG_AE'), model, training_id='h', save_dir='/tmp/mgv_test_exp', lr=1e-4,
                          rc_prob_func_weight=[1.0, 4.0, 4.0], device='cuda:0', batch_size=3, distributed=False)
    tr.optimizer.zero_grad()
    ls = tr.run_batch(batch)
    tr.weighted_loss(ls).backward()
    p = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and 'running_' not in k else v.clone()) for k, v in sd.items()}
    bn = {k: v.clone() for k, v in p.items() if 'running_' in k}
    ob = R.batch_from_arrays(lambda k: arrays[k])
    ols = R.run_batch(p, ctype, ob, training=True, bn_state=bn, p_drop=0.0, s_rounds=2, t_rounds=2)
    R.weighted_loss(ols, [1.0, 4.0, 4.0]).backward()
    for k in ('recon_loss', 'prob_loss', 'func_loss'):
        close(ls[k], ols[k].detach().numpy(), rtol=1e-4, msg=k)
    for k, q in model.named_parameters():
        ref = p[k].grad
        if q.grad is None:
            assert ref is None or float(ref.abs().max()) < 1e-5, k
            continue
        if ref is None:         # aggregator of a gate type the batch does not contain (AND/OR in a MAJ+NOT MIG)
            assert float(q.grad.abs().max()) == 0.0, k
            continue
        g, ref = q.grad.detach().cpu().numpy(), ref.numpy()
        if 'attn_lin.weight' in k:
            g, ref = g[:, H:], ref[:, H:]
        scale = max(1e-6, float(np.abs(ref).max()))
        # 5e-6 floor: Linear biases in front of a BatchNorm have a mathematically zero gradient (noise on both sides)
        np.testing.assert_allclose(g, ref, rtol=2e-3, atol=grad_atol() * scale + 5e-6, err_msg='grad ' + k)


def test_high_fanout_input_against_the_oracle():
    """A primary input that drives 700 gates (clock/reset-like) and a level-1 gate that drives 500: their lists take the heavy-row paths — neighbour sums of the struct
    stages by a pre-pass, reconstruction-loss and sweep pulls per list segment — and every loss and gradient still equals the oracle's."""
    dev = _dev()
    import deepgate
    from deepgate import synthetic as syn
    from oracle import ref_cpu as R
    H, ctype = 64, 'aig'
    torch.manual_seed(6)
    enc = deepgate.digae_layer.DirectMultiGCNEncoder(dim_feature=6, dim_hidden=H, s_rounds=2, t_rounds=2, layernorm=True)
    model = deepgate.dg_ae_model_aig.Model(struct_encoder=enc, dim_hidden=H)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model.to(dev).train()
    arrays = syn.collate([syn.make_graph(ctype, 1500, 12, 800 + i, n_inputs=24) for i in range(2)])
    rng = np.random.Generator(np.random.PCG64(4))
    gates = np.nonzero(arrays['forward_level'] > 0)[0]
    dst = rng.choice(gates, size=700, replace=False)
    ei = arrays['edge_index']
    have = set((ei[0] * arrays['num_nodes'] + ei[1]).tolist())
    dst = np.array([d for d in dst if (5 * arrays['num_nodes'] + d) not in have])
    # ... and an UPDATED gate of level 1 (an inverter of an input, say) that drives 500 gates of later levels
    lv = arrays['forward_level']
    hub2 = int(np.nonzero(lv == 1)[0][3])
    later = np.nonzero(lv >= 2)[0]
    dst2 = np.array([d for d in rng.choice(later, size=500, replace=False) if (hub2 * arrays['num_nodes'] + d) not in have])
    arrays['edge_index'] = np.concatenate([ei, np.stack([np.full(len(dst), 5, dtype=ei.dtype), dst.astype(ei.dtype)]),
                                           np.stack([np.full(len(dst2), hub2, dtype=ei.dtype), dst2.astype(ei.dtype)])], axis=1)
    batch = deepgate.CircuitBatch.from_arrays(arrays, device=dev)
    tr = deepgate.Trainer(types.SimpleNamespace(model='DG_AE'), model, training_id='hub', save_dir='/tmp/mgv_test_exp', lr=1e-4,
                          rc_prob_func_weight=[1.0, 0.0, 4.0], device='cuda:0', batch_size=2, distributed=False)
    tr.optimizer.zero_grad()
    ls = tr.run_batch(batch)
    plan = batch._mgv_plan
    assert plan.heavy(True)[0] >= 2 and plan.heavy_segments(True, inactive_only=True) is not None      # the heavy paths did run
    assert plan.heavy_segments(True, active_by_level=True) is not None
    tr.weighted_loss(ls).backward()
    p = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and 'running_' not in k else v.clone()) for k, v in sd.items()}
    bn = {k: v.clone() for k, v in p.items() if 'running_' in k}
    ob = R.batch_from_arrays(lambda k: arrays[k])
    ols = R.run_batch(p, ctype, ob, training=True, bn_state=bn, p_drop=0.0, s_rounds=2, t_rounds=2)
    R.weighted_loss(ols, [1.0, 0.0, 4.0]).backward()
    for k in ('recon_loss', 'prob_loss', 'func_loss'):
        close(ls[k], ols[k].detach().numpy(), rtol=1e-4, msg=k)
    for k, q in model.named_parameters():
        ref = p[k].grad
        if q.grad is None or ref is None:
            assert (ref is None or float(ref.abs().max()) < 1e-5) and (q.grad is None or float(q.grad.abs().max()) < 1e-5), k
            continue
        g, ref = q.grad.detach().cpu().numpy(), ref.numpy()
        if 'attn_lin.weight' in k:
            g, ref = g[:, H:], ref[:, H:]
        scale = max(1e-6, float(np.abs(ref).max()))
        # (weights [1, 0, 4]: the probability loss is left out — on a 3,000-node batch one flipped ReLU / L1 sign between the split-
        # precision and the float64 side moves every upstream gradient by ~7e-3, which says nothing about the heavy paths)
        np.testing.assert_allclose(g, ref, rtol=2e-3, atol=2 * grad_atol() * scale + 5e-6, err_msg='grad ' + k)
