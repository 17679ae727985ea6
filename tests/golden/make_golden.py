#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ by running the REFERENCE's own code on CPU.

Runs only in the build container (needs /root/reference; the third-party modules the reference
imports are replaced by the test-only stand-ins in tests/oracle_stubs/, see its README).  The
outputs are plain data (.npz: inputs, parameters, expected outputs/gradients); no reference source
is copied.  Usage:  python tests/golden/make_golden.py

Fixture families:
  g1_<type>.npz   H=16, 2 rounds, layernorm, 2 ragged small graphs, every gate type of the model:
                  full state_dict, eval-mode outputs, train-mode (dropout p forced to 0) losses,
                  gradients of every parameter for loss weights [1,4,4], parameters after one Adam step
  g2_<type>.npz   H=64, 4 rounds, layernorm (the BASELINE shape), aig + xmg, 4 graphs x 256 nodes
  g3_ops.npz      per-operator in/out/grad: encoder half-round, TFMlpAggr level (+GRU), MLP with
                  BatchNorm batch statistics, zero_normalization/L1, inner-product decoder
  g4_vae.npz      DirectedGVAE.sample with the two randn_like draws replayed, KL per trainer.py:146-147
  g5_cfg1.npz     3 consecutive run_batch+Adam steps on BASELINE config 1 with dropout active
                  (loose trajectory check only)
  g6_loader.npz   the reference's own parsers on raw MixGate-layout circuits with shuffled node ids:
                  parser_func.parse_pyg_mlpgate (aig, [2,E] layout) and parser_func_others.parse_pyg_mlpgate
                  (xmg, [E,2] layout) incl. return_order_info levels (utils/dag_utils.py:10-37,80-88)
  g7_ckpt.npz +   a checkpoint written by the reference's Trainer.save after one Adam step (g1 aig setup),
  g7_ckpt_ref_aig.pth  the losses / parameters of the reference's NEXT step after Trainer.load of that file
A family whose .npz would exceed 1 MiB (g2_*, g3_ops) is written as parts <name>.0.npz, <name>.1.npz, ... (save_fixture);
the tests read either form through conftest.load_golden.
"""
import argparse
import importlib.util
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'oracle_stubs'))
sys.path.insert(0, '/root/reference/DG_VAE')

import numpy as np  # noqa: E402
import torch  # noqa: E402

import deepgate  # noqa: E402  (the reference)
import deepgate.digae_layer  # noqa: E402
import deepgate.digvae_model  # noqa: E402
import deepgate.dg_ae_model_aig  # noqa: E402
import deepgate.dg_ae_model_mig  # noqa: E402
import deepgate.dg_ae_model_xag  # noqa: E402
import deepgate.dg_ae_model_xmg  # noqa: E402
from deepgate.arch.mlp import MLP  # noqa: E402
from deepgate.arch.tfmlp import TFMlpAggr  # noqa: E402
from deepgate.utils.dag_utils import subgraph  # noqa: E402
from deepgate.utils.utils import zero_normalization  # noqa: E402
from torch_geometric.data import Data  # noqa: E402  (stand-in)

_spec = importlib.util.spec_from_file_location(
    'mgv_synthetic', os.path.join(ROOT, 'multi-gate-vae_amd', 'deepgate', 'synthetic.py'))
syn = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(syn)

MODEL_MODULES = {
    'aig': deepgate.dg_ae_model_aig, 'mig': deepgate.dg_ae_model_mig,
    'xag': deepgate.dg_ae_model_xag, 'xmg': deepgate.dg_ae_model_xmg,
}
assert deepgate.__file__.startswith('/root/reference'), deepgate.__file__


def to_data(b):
    d = Data()
    d.x = torch.from_numpy(b['x'])
    d.edge_index = torch.from_numpy(b['edge_index'])
    d.gate = torch.from_numpy(b['gate'])
    d.forward_level = torch.from_numpy(b['forward_level'])
    d.forward_index = torch.from_numpy(b['forward_index'])
    d.prob = torch.from_numpy(b['prob'])
    d.tt_pair_index = torch.from_numpy(b['tt_pair_index'])
    d.tt_sim = torch.from_numpy(b['tt_sim'])
    return d


def build_model(ctype, H, R, seed):
    torch.manual_seed(seed)
    enc = deepgate.digae_layer.DirectMultiGCNEncoder(
        dim_hidden=H, dim_feature=6, enable_reverse=True, s_rounds=R, t_rounds=R, layernorm=True)
    model = MODEL_MODULES[ctype].Model(struct_encoder=enc, dim_hidden=H, enable_encode=True,
                                       enable_reverse=True)
    # default init leaves LN/BN affine at (1,0) and BN running stats at (0,1); perturb them so a
    # swapped gamma/beta or an ignored running statistic cannot pass
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, (torch.nn.LayerNorm, torch.nn.BatchNorm1d)):
                m.weight.add_(0.2 * torch.randn(m.weight.shape, generator=g))
                m.bias.add_(0.2 * torch.randn(m.bias.shape, generator=g))
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.add_(0.1 * torch.randn(m.running_mean.shape, generator=g))
                m.running_var.mul_(1.0 + 0.3 * torch.rand(m.running_var.shape, generator=g))
    return model


def set_dropout(model, p):
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = p


def sd_arrays(prefix, sd):
    return {prefix + k: v.detach().cpu().numpy().copy() for k, v in sd.items()}


def make_trainer(model, weights, lr):
    args = types.SimpleNamespace(model='DG_AE')
    tmp = tempfile.mkdtemp(prefix='mgv_golden_')
    tr = deepgate.Trainer(args, model, training_id='g', save_dir=tmp, lr=lr,
                          rc_prob_func_weight=list(weights), device='cpu', batch_size=1,
                          distributed=False)
    return tr


def model_fixture(ctype, H, R, graphs, seed, with_adam):
    batch = syn.collate(graphs)
    model = build_model(ctype, H, R, seed)
    mod = MODEL_MODULES[ctype]
    neg = torch.from_numpy(batch['neg_edge_index'])
    mod.negative_sampling = lambda *a, **k: neg  # recon_loss() draws negatives through this name
    out = {'meta_type': np.array(ctype), 'meta_H': np.array(H), 'meta_R': np.array(R),
           'meta_weights': np.array([1.0, 4.0, 4.0], dtype=np.float32), 'meta_lr': np.array(1e-4)}
    for k in ('x', 'edge_index', 'gate', 'forward_level', 'forward_index', 'prob', 'tt_pair_index',
              'tt_sim', 'neg_edge_index', 'graph_ptr'):
        out['in_' + k] = batch[k]
    out.update(sd_arrays('param_', model.state_dict()))

    # ---- eval mode: forward outputs and losses with BatchNorm running statistics
    model.eval()
    d = to_data(batch)
    enc = getattr(model, {'aig': 'struct_encoder'}.get(ctype, ctype + '_struct_encoder'))
    with torch.no_grad():
        one_hot = torch.nn.functional.one_hot(d.x[:, 1].to(int), num_classes=6)
        s, t = enc(one_hot, one_hot, d.edge_index)
        hs, hf = model(d)
        prob = model.pred_prob(hf)
        rl, pred_bin, gt_bin = model.recon_loss(hs, d.edge_index, neg)
    out.update(eval_s=s.numpy(), eval_t=t.numpy(), eval_hs=hs.numpy(), eval_hf=hf.numpy(),
               eval_prob=prob.numpy(), eval_recon=rl.numpy(), eval_pred_bin=pred_bin.numpy(),
               eval_gt_bin=gt_bin.numpy())

    # ---- train mode, dropout p forced to 0: Trainer.run_batch -> weighted loss -> backward -> Adam
    model.train()
    set_dropout(model, 0.0)
    tr = make_trainer(model, [1.0, 4.0, 4.0], 1e-4)
    tr.optimizer.zero_grad()
    torch.manual_seed(seed + 7)           # the edge permutation in general_train_test_split_edges
    ls = tr.run_batch(to_data(batch))
    loss = (tr.rc_prob_func_weight[0] * ls['recon_loss'] + tr.rc_prob_func_weight[1] * ls['prob_loss']
            + tr.rc_prob_func_weight[2] * ls['func_loss'])
    loss.backward()
    out.update(train_recon=ls['recon_loss'].detach().numpy(), train_prob_loss=ls['prob_loss'].detach().numpy(),
               train_func_loss=ls['func_loss'].detach().numpy(), train_loss=loss.detach().numpy(),
               train_pred_bin_sum=np.array(int(ls['pred_bin'].sum())),
               train_gt_bin_sum=np.array(int(ls['gt_bin'].sum())))
    for k, p in model.named_parameters():
        out['grad_' + k] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy().copy()
    if with_adam:
        tr.optimizer.step()
        out.update(sd_arrays('after_', model.state_dict()))
    return out


def g1(ctype):
    graphs = [syn.make_graph(ctype, 48, 7, 9100 + i, n_inputs=6) for i in range(1)]
    graphs.append(syn.make_graph(ctype, 40, 7, 9200, n_inputs=5))
    return model_fixture(ctype, 16, 2, graphs, seed=11, with_adam=True)


def g2(ctype):
    graphs = [syn.make_graph(ctype, 256, 12, 9300 + i, n_inputs=16) for i in range(4)]
    return model_fixture(ctype, 64, 4, graphs, seed=12, with_adam=False)


def g3_ops():
    out = {}
    H = 64
    torch.manual_seed(21)
    g = syn.make_graph('xmg', 96, 6, 9400, n_inputs=12)
    ei = torch.from_numpy(g['edge_index'])
    N = g['num_nodes']
    # -- encoder half rounds (AggConv -> GRU([msg,x]) -> LayerNorm), forward and reversed edges
    enc = deepgate.digae_layer.MultiGCNEncoder(1, H, 6, True, True)
    with torch.no_grad():
        enc.ln.weight.add_(0.2 * torch.randn(H))
        enc.ln.bias.add_(0.2 * torch.randn(H))
    x1h = torch.nn.functional.one_hot(torch.from_numpy(g['x'])[:, 1].to(int), num_classes=6)
    h0 = torch.randn(1, N, H, requires_grad=True)
    msg = enc.aggr(h0, ei)
    _, h1 = enc.update(torch.cat([msg, x1h.unsqueeze(0)], dim=-1), h0)
    h1n = enc.ln(h1)
    r_ei = torch.stack([ei[1], ei[0]], dim=0)
    msg_r = enc.aggr_r(h1n, r_ei)
    _, h2 = enc.update_r(torch.cat([msg_r, x1h.unsqueeze(0)], dim=-1), h1n)
    h2n = enc.ln(h2)
    up = torch.randn(1, N, H)
    (h2n * up).sum().backward()
    out.update(sd_arrays('enc_param_', enc.state_dict()))
    out.update(enc_edge_index=g['edge_index'], enc_x=x1h.numpy(), enc_h0=h0.detach().numpy()[0],
               enc_msg=msg.detach().numpy()[0], enc_h1_pre_ln=h1.detach().numpy()[0],
               enc_h1=h1n.detach().numpy()[0], enc_h2=h2n.detach().numpy()[0], enc_up=up.numpy()[0],
               enc_grad_h0=h0.grad.numpy()[0])
    for k, p in enc.named_parameters():
        out['enc_grad_' + k] = p.grad.numpy().copy()

    # -- one functional level: TFMlpAggr over the in-edges of a node set (fan-in 1..5), then GRU
    torch.manual_seed(22)
    Nn = 40
    src, dst = [], []
    rng = np.random.Generator(np.random.PCG64(5))
    targets = np.arange(20, 36)
    for i, n in enumerate(targets):
        deg = 1 + (i % 5)
        for s_ in rng.choice(20, size=deg, replace=False):
            src.append(int(s_)); dst.append(int(n))
    # unrelated edges into other nodes must be ignored by the level
    src += [1, 2, 3]; dst += [37, 38, 39]
    lei = torch.tensor([src, dst], dtype=torch.long)
    aggr = TFMlpAggr(2 * H, H)
    gru = torch.nn.GRU(H, H)
    node_state = torch.randn(Nn, 2 * H, requires_grad=True)
    hprev = torch.randn(Nn, H, requires_grad=True)     # non-zero h0 (num_rounds > 1 case)
    l_node = torch.from_numpy(targets)
    sub_ei, _ = subgraph(l_node, lei, dim=1)
    m = aggr(node_state, sub_ei, None)
    lm = torch.index_select(m, 0, l_node)
    _, hnew = gru(lm.unsqueeze(0), torch.index_select(hprev, 0, l_node).unsqueeze(0))
    hnew = hnew.squeeze(0)
    upl = torch.randn(len(targets), H)
    (hnew * upl).sum().backward()
    out.update(sd_arrays('lvl_aggr_', aggr.state_dict()))
    out.update(sd_arrays('lvl_gru_', gru.state_dict()))
    out.update(lvl_edge_index=lei.numpy(), lvl_nodes=targets, lvl_node_state=node_state.detach().numpy(),
               lvl_hprev=hprev.detach().numpy(), lvl_msg=lm.detach().numpy(), lvl_hnew=hnew.detach().numpy(),
               lvl_up=upl.numpy(), lvl_grad_node_state=node_state.grad.numpy(), lvl_grad_hprev=hprev.grad.numpy())
    for k, p in aggr.named_parameters():
        out['lvl_grad_aggr_' + k] = p.grad.numpy().copy()
    for k, p in gru.named_parameters():
        out['lvl_grad_gru_' + k] = p.grad.numpy().copy()

    # -- the same level with h0 = 0 (num_rounds = 1: a node is updated once, from a zero state)
    aggr.zero_grad(); gru.zero_grad()
    ns0 = node_state.detach().clone().requires_grad_(True)
    m0 = aggr(ns0, sub_ei, None)
    lm0 = torch.index_select(m0, 0, l_node)
    _, hnew0 = gru(lm0.unsqueeze(0), torch.zeros(1, len(targets), H))
    hnew0 = hnew0.squeeze(0)
    (hnew0 * upl).sum().backward()
    out.update(lvl0_hnew=hnew0.detach().numpy(), lvl0_grad_node_state=ns0.grad.numpy())
    for k, p in aggr.named_parameters():
        out['lvl0_grad_aggr_' + k] = p.grad.numpy().copy()
    for k, p in gru.named_parameters():
        out['lvl0_grad_gru_' + k] = p.grad.numpy().copy()

    # -- readout MLP with BatchNorm batch statistics (dropout p forced to 0), clamp, L1
    torch.manual_seed(23)
    mlp = MLP(H, 32, 1, num_layer=3, p_drop=0.2, norm_layer='batchnorm', act_layer='relu')
    set_dropout(mlp, 0.0)
    with torch.no_grad():
        for mm in mlp.modules():
            if isinstance(mm, torch.nn.BatchNorm1d):
                mm.weight.add_(0.2 * torch.randn(32)); mm.bias.add_(0.2 * torch.randn(32))
    mlp.train()
    hin = torch.randn(300, H, requires_grad=True)
    tgt = torch.rand(300, 1)
    pr = torch.clamp(mlp(hin), min=0.0, max=1.0)
    l1 = torch.nn.L1Loss()(pr, tgt)
    l1.backward()
    out.update(sd_arrays('mlp_param_', {k: v for k, v in mlp.state_dict().items()}))
    out.update(mlp_in=hin.detach().numpy(), mlp_target=tgt.numpy(), mlp_prob=pr.detach().numpy(),
               mlp_l1=l1.detach().numpy(), mlp_grad_in=hin.grad.numpy())
    for k, p in mlp.named_parameters():
        out['mlp_grad_' + k] = p.grad.numpy().copy()
    sd_after = mlp.state_dict()
    out['mlp_after_running_mean1'] = sd_after['fc.1.running_mean'].numpy().copy()
    out['mlp_after_running_var1'] = sd_after['fc.1.running_var'].numpy().copy()
    out['mlp_after_running_mean5'] = sd_after['fc.5.running_mean'].numpy().copy()
    out['mlp_after_running_var5'] = sd_after['fc.5.running_var'].numpy().copy()

    # -- functional-similarity loss: cosine distance -> zero_normalization -> L1 (trainer.py:158-163)
    torch.manual_seed(24)
    hf = torch.randn(50, H, requires_grad=True)
    pairs = torch.randint(0, 50, (2, 33))
    tts = torch.rand(33)
    dis = 1 - torch.cosine_similarity(hf[pairs[0]], hf[pairs[1]], eps=1e-8)
    fl = torch.nn.L1Loss()(zero_normalization(dis), zero_normalization(tts))
    fl.backward()
    out.update(fl_hf=hf.detach().numpy(), fl_pairs=pairs.numpy(), fl_tt=tts.numpy(), fl_dis=dis.detach().numpy(),
               fl_loss=fl.detach().numpy(), fl_grad_hf=hf.grad.numpy())

    # -- directed inner-product decoder (digae_layer.py:26-33)
    torch.manual_seed(25)
    dec = deepgate.digae_layer.DirectedInnerProductDecoder()
    s = torch.randn(30, H); t = torch.randn(30, H)
    dei = torch.randint(0, 30, (2, 45))
    out.update(dec_s=s.numpy(), dec_t=t.numpy(), dec_edge_index=dei.numpy(),
               dec_sig=dec(s, t, dei, sigmoid=True).numpy(), dec_raw=dec(s, t, dei, sigmoid=False).numpy(),
               dec_all=dec.forward_all(s, t).numpy())
    return out


def g4_vae():
    H = 64
    torch.manual_seed(31)
    enc = deepgate.digae_layer.DirectMultiGCNEncoder(dim_hidden=H, dim_feature=6, s_rounds=1, t_rounds=1,
                                                     layernorm=True)
    vae = deepgate.digvae_model.DirectedGVAE(enc, H, deepgate.digae_layer.DirectedInnerProductDecoder())
    s = torch.randn(70, H, requires_grad=True)
    t = torch.randn(70, H, requires_grad=True)
    torch.manual_seed(32)
    eps_s = torch.randn(70, H)      # replay of the two randn_like draws, s first then t
    eps_t = torch.randn(70, H)
    torch.manual_seed(32)
    zs, zt = vae.sample(s, t)
    n = s.size(0)
    s_kl = -0.5 / n * (1 + 2 * vae.s_logstd - vae.s_mu ** 2 - torch.exp(vae.s_logstd) ** 2).sum(1).mean()
    t_kl = -0.5 / n * (1 + 2 * vae.t_logstd - vae.t_mu ** 2 - torch.exp(vae.t_logstd) ** 2).sum(1).mean()
    up_s = torch.randn(70, H); up_t = torch.randn(70, H)
    ((zs * up_s).sum() + (zt * up_t).sum() + 3.0 * (s_kl + t_kl)).backward()
    out = {k: v.detach().numpy().copy() for k, v in vae.state_dict().items() if k.startswith('fc_')}
    out = {'param_' + k: v for k, v in out.items()}
    out.update(s=s.detach().numpy(), t=t.detach().numpy(), eps_s=eps_s.numpy(), eps_t=eps_t.numpy(),
               sample_s=zs.detach().numpy(), sample_t=zt.detach().numpy(), s_kl=s_kl.detach().numpy(),
               t_kl=t_kl.detach().numpy(), up_s=up_s.numpy(), up_t=up_t.numpy(), kl_weight=np.array(3.0),
               grad_s=s.grad.numpy(), grad_t=t.grad.numpy())
    for k, p in vae.named_parameters():
        if k.startswith('fc_'):
            out['grad_' + k] = p.grad.numpy().copy()
    return out


def g5_cfg1():
    batch = syn.make_batch(1)
    model = build_model('aig', 64, 4, seed=41)
    neg = torch.from_numpy(batch['neg_edge_index'])
    deepgate.dg_ae_model_aig.negative_sampling = lambda *a, **k: neg
    model.train()                         # dropout p=0.2 active
    tr = make_trainer(model, [1.0, 4.0, 4.0], 1e-4)
    out = sd_arrays('param_', model.state_dict())
    losses = []
    torch.manual_seed(42)
    for _ in range(3):
        tr.optimizer.zero_grad()
        ls = tr.run_batch(to_data(batch))
        loss = ls['recon_loss'] + 4.0 * ls['prob_loss'] + 4.0 * ls['func_loss']
        loss.backward()
        tr.optimizer.step()
        losses.append([float(ls['recon_loss']), float(ls['prob_loss']), float(ls['func_loss'])])
    out['losses'] = np.asarray(losses, dtype=np.float64)
    out['meta_config'] = np.array(1)
    return out


def _raw_circuit(ctype, seed):
    """A synthetic circuit in the raw MixGate layout with SHUFFLED node ids (levels are not contiguous id ranges)."""
    g = syn.make_graph(ctype, 100, 9, seed, n_inputs=10)
    n = g['num_nodes']
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    perm = rng.permutation(n)                       # new id of old node i
    inv = np.argsort(perm)
    gate = g['gate'].reshape(-1)[inv].astype(np.int64)
    x = np.stack([np.arange(n), gate], 1).astype(np.float64)          # column 0 = node id, column 1 = gate id
    ei = perm[g['edge_index']]
    order = rng.permutation(ei.shape[1])            # edge order shuffled too
    ei = ei[:, order]
    tp = perm[g['tt_pair_index']]
    return x, ei, g['prob'].reshape(-1)[inv].astype(np.float32), g['tt_sim'], tp


def g6_loader():
    from deepgate import parser_func, parser_func_others
    out = {}
    for tag, ctype, fn, transposed in (('aig', 'aig', parser_func.parse_pyg_mlpgate, False),
                                       ('xmg', 'xmg', parser_func_others.parse_pyg_mlpgate, True)):
        x, ei, prob, tts, tp = _raw_circuit(ctype, 9700)
        ei_in = ei.T.copy() if transposed else ei
        tp_in = tp.T.copy() if transposed else tp
        g = fn(x, ei_in, prob, tts, tp_in)
        out.update({tag + '_in_x': x, tag + '_in_edge_index': ei_in, tag + '_in_prob': prob, tag + '_in_tt_sim': tts,
                    tag + '_in_tt_pair_index': tp_in,
                    tag + '_x': g.x.numpy(), tag + '_edge_index': g.edge_index.numpy(),
                    tag + '_forward_level': g.forward_level.numpy(), tag + '_forward_index': g.forward_index.numpy(),
                    tag + '_backward_level': g.backward_level.numpy(), tag + '_prob': g.prob.numpy(),
                    tag + '_tt_pair_index': g.tt_pair_index.numpy(), tag + '_tt_sim': g.tt_sim.numpy()})
        if hasattr(g, 'gate') and g.gate is not None:
            out[tag + '_gate'] = g.gate.numpy()
    return out


def g7_ckpt():
    """Reference Trainer: step, save, (fresh trainer) load, step -> what a drop-in must reproduce from the same file."""
    ctype, H, R, seed = 'aig', 16, 2, 11
    graphs = [syn.make_graph(ctype, 48, 7, 9100, n_inputs=6), syn.make_graph(ctype, 40, 7, 9200, n_inputs=5)]
    batch = syn.collate(graphs)
    neg = torch.from_numpy(batch['neg_edge_index'])
    MODEL_MODULES[ctype].negative_sampling = lambda *a, **k: neg

    def step(tr):
        tr.optimizer.zero_grad()
        torch.manual_seed(seed + 7)
        ls = tr.run_batch(to_data(batch))
        (ls['recon_loss'] + 4.0 * ls['prob_loss'] + 4.0 * ls['func_loss']).backward()
        tr.optimizer.step()
        return [float(ls['recon_loss']), float(ls['prob_loss']), float(ls['func_loss'])]

    model = build_model(ctype, H, R, seed)
    model.train(); set_dropout(model, 0.0)
    tr = make_trainer(model, [1.0, 4.0, 4.0], 1e-4)
    l1 = step(tr)
    tr.model_epoch = 3
    path = os.path.join(HERE, 'g7_ckpt_ref_aig.pth')
    tr.save(path)
    model2 = build_model(ctype, H, R, seed + 100)          # different init: everything must come from the file
    model2.train(); set_dropout(model2, 0.0)
    tr2 = make_trainer(model2, [1.0, 4.0, 4.0], 1e-4)
    tr2.load(path)
    l2 = step(tr2)
    out = {'meta_type': np.array(ctype), 'meta_H': np.array(H), 'meta_R': np.array(R), 'meta_epoch': np.array(3),
           'losses_step1': np.asarray(l1), 'losses_step2': np.asarray(l2)}
    for k in ('x', 'edge_index', 'gate', 'forward_level', 'forward_index', 'prob', 'tt_pair_index', 'tt_sim', 'neg_edge_index', 'graph_ptr'):
        out['in_' + k] = batch[k]
    out.update(sd_arrays('saved_', model.state_dict()))
    out.update(sd_arrays('after2_', model2.state_dict()))
    osd = tr2.optimizer.state_dict()['state']
    names = [k for k, _ in model2.named_parameters()]
    for i, k in enumerate(names):
        if i in osd:
            out['adam2_exp_avg_' + k] = osd[i]['exp_avg'].numpy().copy()
            out['adam2_exp_avg_sq_' + k] = osd[i]['exp_avg_sq'].numpy().copy()
            out['adam2_step'] = np.array(float(osd[i]['step']))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default='')
    a = ap.parse_args()
    jobs = {}
    for t in ('aig', 'mig', 'xag', 'xmg'):
        jobs['g1_' + t] = (lambda t=t: g1(t))
    for t in ('aig', 'xmg'):
        jobs['g2_' + t] = (lambda t=t: g2(t))
    jobs['g3_ops'] = g3_ops
    jobs['g4_vae'] = g4_vae
    jobs['g5_cfg1'] = g5_cfg1
    jobs['g6_loader'] = g6_loader
    jobs['g7_ckpt'] = g7_ckpt
    for name, fn in jobs.items():
        if a.only and a.only not in name:
            continue
        arrs = fn()
        paths = save_fixture(name, arrs)
        print('%-10s %4d arrays %8.1f KB in %d file(s)' % (name, len(arrs), sum(os.path.getsize(p) for p in paths) / 1024, len(paths)))


PART_BYTES = 900 * 1024     # a committed file stays under 1 MiB


def save_fixture(name, arrs):
    """<name>.npz, or — when the compressed arrays exceed PART_BYTES — consecutive parts <name>.0.npz, <name>.1.npz, ... of whole
    arrays in their order (tests/conftest.py load_golden merges them).  Returns the paths written."""
    import glob
    import zlib
    parts, cur, size = [], {}, 0
    for k, v in arrs.items():
        n = len(zlib.compress(np.asarray(v).tobytes()))
        if cur and size + n > PART_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += n
    parts.append(cur)
    for old in glob.glob(os.path.join(HERE, glob.escape(name) + '.[0-9]*.npz')) + glob.glob(os.path.join(HERE, glob.escape(name) + '.npz')):
        os.remove(old)
    paths = [os.path.join(HERE, name + '.npz')] if len(parts) == 1 else [os.path.join(HERE, '%s.%d.npz' % (name, i)) for i in range(len(parts))]
    for path, part in zip(paths, parts):
        np.savez_compressed(path, **part)
        assert os.path.getsize(path) < 1 << 20, path
    return paths


if __name__ == '__main__':
    main()
