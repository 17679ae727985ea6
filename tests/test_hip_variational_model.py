"""GPU tests of Model(variational=True) through the public surface: the training step with the variational link heads on the second
stream (Trainer.overlap, kl_weight), kl_loss / latent, the decoders on the posterior means, the two routes of ops.var_head, and that
a default model launches what it launched before.  Batch: two synthetic AIGs of 256 nodes, H = 64."""
import collections
import itertools
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_ref as DR  # noqa: E402
import var_head_ref as VR  # noqa: E402

pytestmark = pytest.mark.gpu

H = 64
WEIGHTS = [1.0, 4.0, 4.0]
KL_WEIGHT = 0.5
F64, F32 = torch.float64, torch.float32
HEAD_LAUNCHES = {'mgv_var_head_fwd_x3': 1, 'mgv_var_head_bwd_x3': 1, 'mgv_wpack_bf16x3': 4}      # two packs forward, two transposed backward


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _batch(dev):
    import deepgate
    from deepgate import synthetic as syn
    graphs = [syn.make_graph('aig', 256, 8, 6100 + i, n_inputs=16) for i in range(2)]
    for g in graphs:
        del g['neg_edge_index']
    return deepgate.CircuitBatch.from_arrays(syn.collate(graphs), device=dev)


def _model(dev, variational, seed=9):
    import deepgate
    torch.manual_seed(seed)
    enc = deepgate.digae_layer.DirectMultiGCNEncoder(dim_feature=6, dim_hidden=H, s_rounds=2, t_rounds=2, layernorm=True)
    model = deepgate.dg_ae_model_aig.Model(struct_encoder=enc, dim_hidden=H, **({'variational': True} if variational else {}))
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return model.to(dev).train()


_RUNS = {}


def _runs(kind, monkeypatch):
    """kind: 'var' (fused head), 'composed' (ops.VAR_HEAD_FUSED off) or 'plain' (variational=False).  The step (run_batch,
    weighted_loss, backward) twice with overlap on and twice with it off, every step from the same torch seed (the head's noise
    seed is drawn from torch's CPU generator) and the same sampled negatives."""
    if kind in _RUNS:
        return _RUNS[kind]
    dev = _dev()
    import deepgate
    from deepgate import _hip, ops, sampling
    monkeypatch.setattr(ops, 'VAR_HEAD_FUSED', kind != 'composed')
    model = _model(dev, kind != 'plain')
    batch = _batch(dev)
    tr = deepgate.Trainer(types.SimpleNamespace(model='DG_AE', kl_weight=KL_WEIGHT), model, training_id='var', save_dir='/tmp/mgv_test_exp', lr=1e-4,
                          rc_prob_func_weight=WEIGHTS, device='cuda:0', batch_size=2, distributed=False)
    assert tr.kl_weight == KL_WEIGHT
    record = []
    real = _hip.call

    def shim(name, *args):
        record.append((name, _hip.stream().value))
        return real(name, *args)
    monkeypatch.setattr(_hip, 'call', shim)

    def step(overlap):
        monkeypatch.setattr(sampling, '_CALLS', itertools.count())
        torch.manual_seed(123)
        tr.overlap = overlap
        tr.optimizer.zero_grad()
        del record[:]
        ls = tr.run_batch(batch, want_pred=False)
        tr.weighted_loss(ls).backward()
        if tr._branch is not None:
            tr._branch.join()
        torch.cuda.synchronize()
        return {'launches': list(record), 'kl': ls['kl_loss'].detach().clone() if 'kl_loss' in ls else None,
                'losses': [ls[k].detach().clone() for k in ('recon_loss', 'prob_loss', 'func_loss')],
                'grads': {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}}

    step(True), step(True)
    out = {'on': [step(True), step(True)], 'off': [step(False), step(False)], 'main': _hip.stream().value}
    _RUNS[kind] = out
    return out


def test_two_identical_variational_steps_give_identical_bits(monkeypatch):
    r = _runs('var', monkeypatch)
    heads = ['fc_%s_%s.%s' % (h, m, p) for h in 'st' for m in ('mu', 'logstd') for p in ('weight', 'bias')]
    for setting in ('on', 'off'):
        a, b = r[setting]
        assert set(heads) <= set(a['grads']) and a['grads'].keys() == b['grads'].keys()
        diff = [k for k in a['grads'] if not torch.equal(a['grads'][k], b['grads'][k])]
        assert not diff, (setting, diff)
        assert torch.equal(a['kl'], b['kl']) and all(torch.equal(x, y) for x, y in zip(a['losses'], b['losses']))
        assert all(float(a['grads'][k].abs().max()) > 0 for k in heads)
        assert bool(torch.isfinite(a['kl'])) and float(a['kl']) > 0
    # the same kernels on the same inputs with overlap on and off
    assert torch.equal(r['on'][0]['kl'], r['off'][0]['kl'])
    assert all(torch.equal(x, y) for x, y in zip(r['on'][0]['losses'], r['off'][0]['losses']))


def test_the_head_stands_on_the_side_stream_between_hs_decompose_and_the_sampler(monkeypatch):
    r = _runs('var', monkeypatch)
    on, off, main = r['on'][0]['launches'], r['off'][0]['launches'], r['main']
    assert {s for _, s in off} == {main}
    side = [name for name, s in on if s != main]
    assert side.count('mgv_var_head_fwd_x3') == 1 and side.count('mgv_var_head_bwd_x3') == 1
    assert not any(name.startswith('mgv_var_head') or name.startswith('mgv_reparam') for name, s in on if s == main)
    fwd, bwd, loss = side.index('mgv_var_head_fwd_x3'), side.index('mgv_var_head_bwd_x3'), side.index('mgv_recon_step_csr')
    dec_fwd = side.index('mgv_linear_fwd_x3')
    dec_bwd = max(i for i, n in enumerate(side) if n in ('mgv_linear_bwd_x3', 'mgv_linear_wgrad_x3'))
    assert dec_fwd < fwd < loss < bwd < dec_bwd, side
    assert not any(n.startswith('mgv_neg') for n in side[:fwd])                  # the sampler comes behind the head
    assert collections.Counter(n for n, _ in on) == collections.Counter(n for n, _ in off)


def test_a_default_model_launches_what_it_did_and_the_head_adds_only_its_own(monkeypatch):
    plain, var = _runs('plain', monkeypatch), _runs('var', monkeypatch)
    for setting in ('on', 'off'):
        p = [n for n, _ in plain[setting][0]['launches']]
        v = [n for n, _ in var[setting][0]['launches']]
        assert not any('var_head' in n or 'reparam' in n for n in p)
        assert plain[setting][0]['kl'] is None
        extra = collections.Counter(v) - collections.Counter(p)
        assert dict(extra) == HEAD_LAUNCHES and not collections.Counter(p) - collections.Counter(v), extra
        rest = list(v)
        for name, k in HEAD_LAUNCHES.items():
            if name != 'mgv_wpack_bf16x3':
                rest.remove(name)
        i = rest.index('mgv_recon_step_csr')
        # the head's four packs stand around the loss on the branch: two before it, two behind it
        assert [n for n in rest if n != 'mgv_wpack_bf16x3'] == [n for n in p if n != 'mgv_wpack_bf16x3'], setting
        assert i > 0
    side_p = [n for n, s in plain['on'][0]['launches'] if s != plain['main']]
    side_v = [n for n, s in var['on'][0]['launches'] if s != var['main']]
    assert [n for n in side_v if 'var_head' not in n and n != 'mgv_wpack_bf16x3'] == [n for n in side_p if n != 'mgv_wpack_bf16x3']


def test_the_switch_takes_the_composed_route(monkeypatch):
    r = _runs('composed', monkeypatch)
    names = collections.Counter(n for n, _ in r['on'][0]['launches'])
    assert names['mgv_reparam_fwd'] == 2 and names['mgv_reparam_bwd'] == 2 and names['mgv_var_head_fwd_x3'] == 0
    fused = _runs('var', monkeypatch)
    # the same function: same noise (seed pair, element numbering), losses within the bf16x3 products' error of each other
    for a, b in zip(r['off'][0]['losses'], fused['off'][0]['losses']):
        assert abs(float(a) - float(b)) <= 8 * 2.0 ** -17 * max(abs(float(b)), 1.0)
    assert abs(float(r['off'][0]['kl']) - float(fused['off'][0]['kl'])) <= 8 * 2.0 ** -17 * abs(float(fused['off'][0]['kl'])) * 4


def _restated(model, st, eps, gZ, gkl, sample=1):
    Wp = [torch.cat([getattr(model, 'fc_%s_mu' % h).weight, getattr(model, 'fc_%s_logstd' % h).weight]).detach().cpu() for h in 'st']
    bp = [torch.cat([getattr(model, 'fc_%s_mu' % h).bias, getattr(model, 'fc_%s_logstd' % h).bias]).detach().cpu() for h in 'st']
    kw = dict(eps=eps.cpu(), seed=0, sample=sample, gZ=gZ.cpu() if gZ is not None else None, gkl=gkl, H=H)
    return VR.var_head(st.cpu(), Wp, bp, **kw), VR.var_head(st.cpu(), Wp, bp, dtype=F32, mm='x3', **kw)


def test_head_gradients_and_dhs_against_the_restatement_on_the_devices_own_st_and_gz(monkeypatch):
    """recon_loss + kl_weight * kl under autograd with injected noise; st and gZ are read where ops.var_head sees them, the float64
    restatement runs on exactly those, and dhs = dST W_decompose continues it through the hs_decompose backward."""
    dev = _dev()
    from deepgate import ops
    model, batch = _model(dev, True), _batch(dev)
    with torch.no_grad():
        hs, _ = model(batch)
    hs = hs.detach().requires_grad_(True)
    N = hs.shape[0]
    seen = {}
    real = ops.var_head

    def spy(st, heads, **kw):
        z, kl = real(st, heads, **kw)
        seen['st'] = st.detach().clone()
        z.register_hook(lambda g: seen.__setitem__('gZ', g.detach().clone()))
        return z, kl
    monkeypatch.setattr(ops, 'var_head', spy)
    eps = torch.randn(N, 2 * H, generator=torch.Generator().manual_seed(3)).to(dev)
    loss = model.recon_loss(hs, batch.edge_index, None, want_pred=False, plan=batch._mgv_plan, eps=eps, sample=True)[0]
    s_kl, t_kl = model.kl_loss()
    (loss + KL_WEIGHT * (s_kl + t_kl)).backward()
    torch.cuda.synchronize()
    gk = KL_WEIGHT * (-0.5 / N / N)
    r64, rk = _restated(model, seen['st'], eps, seen['gZ'], (gk, gk))
    tau = VR.taus(r64, rk)
    g = {n: p.grad.detach().cpu() for n, p in model.named_parameters() if n.startswith('fc_')}
    got = {}
    for h in 'st':
        got['dWp_' + h] = torch.cat([g['fc_%s_mu.weight' % h], g['fc_%s_logstd.weight' % h]])
        got['dbp_' + h] = torch.cat([g['fc_%s_mu.bias' % h], g['fc_%s_logstd.bias' % h]])
    got['kl'] = torch.stack([s_kl, t_kl]).detach().cpu().double() / (-0.5 / N / N)
    bad = []
    for k, v in got.items():
        q = DR.ratio(v, r64[k], r64['S'][k])
        print('VM %s %.2g/%.2g' % (k, q, tau[k] + 2.0 ** -23))
        if not q <= tau[k] + 2.0 ** -23:           # (the sums are handed on as float32, and scaled once more)
            bad.append((k, q, tau[k]))
    # dhs = dST W (hs_decompose's input gradient; nothing else consumes hs here): one more bf16x3 product on top of dST
    W = model.hs_decompose.weight.detach().cpu().double()
    ref, S = r64['dST'] @ W, r64['S']['dST'] @ W.abs()
    q = DR.ratio(hs.grad.cpu(), ref, S)
    bound = tau['dST'] + 8 * DR.FLOOR['x3']
    print('VM dhs %.2g/%.2g' % (q, bound))
    if not q <= bound:
        bad.append(('dhs', q, bound))
    assert not bad, bad


def test_kl_loss_equals_the_sums_restated_from_latent():
    """-0.5 / N^2 times sum(1 + 2 ls - mu^2 - e^2ls) over latent()'s own values in float64.  The kernel adds float32 terms of at most
    four roundings and a float32 exp squared (2 ulp): within 8 x 2^-24 of the sum of the terms' magnitudes, and the float32 result."""
    dev = _dev()
    model, batch = _model(dev, True), _batch(dev)
    model.eval()
    with torch.no_grad():
        hs, _ = model(batch)
        model.recon_loss(hs, batch.edge_index, None, want_pred=False, plan=batch._mgv_plan)
        kl = [float(k) for k in model.kl_loss()]
        mu_s, ls_s, mu_t, ls_t = (t.double().cpu() for t in model.latent(hs))
    N = hs.shape[0]
    assert mu_s.shape == (N, H) and ls_t.shape == (N, H)
    for got, mu, ls in ((kl[0], mu_s, ls_s), (kl[1], mu_t, ls_t)):
        want = -0.5 / N / N * float((1 + 2 * ls - mu * mu - torch.exp(2 * ls)).sum())
        mag = 0.5 / N / N * float((1 + 2 * ls.abs() + mu * mu + torch.exp(2 * ls)).sum())
        assert abs(got - want) <= 9 * 2.0 ** -24 * mag, (got, want, mag)


def test_eval_mode_decodes_the_means_and_the_link_tools_use_them():
    dev = _dev()
    from deepgate import pairs
    model, batch = _model(dev, True), _batch(dev)
    with torch.no_grad():
        hs, _ = model(batch)
        neg = torch.randint(0, hs.shape[0], (2, 700), generator=torch.Generator().manual_seed(1)).to(dev)
        model.eval()
        a = model.recon_loss(hs, batch.edge_index, neg, want_pred=False)[0]
        b = model.recon_loss(hs, batch.edge_index, neg, want_pred=False)[0]
        assert torch.equal(a, b)                                   # no noise: sample=None means self.training
        model.train()
        c = model.recon_loss(hs, batch.edge_index, neg, want_pred=False, seed=5)[0]
        d = model.recon_loss(hs, batch.edge_index, neg, want_pred=False, seed=5)[0]
        e = model.recon_loss(hs, batch.edge_index, neg, want_pred=False, seed=6)[0]
        assert torch.equal(c, d) and not torch.equal(c, e) and not torch.equal(a, c)
        f = model.recon_loss(hs, batch.edge_index, neg, want_pred=False, sample=False)[0]
        assert torch.equal(a, f)
        model.eval()
        mu_s, _, mu_t, _ = model.latent(hs)
        idx, score, n_above = model.predict_links(hs, 4, graph_ptr=batch.graph_ptr)
        idx2, score2, n2 = pairs.pair_topk(mu_s, mu_t, 4, graph_ptr=batch.graph_ptr, sigmoid=True, threshold=0.5, skip_self=True)
        assert torch.equal(idx, idx2) and torch.equal(score, score2) and torch.equal(n_above, n2)
        rec = model.link_metrics(hs, batch.edge_index, neg).tolist()
        assert 0.0 <= rec[0] <= 1.0 and 0.0 <= rec[1] <= 1.0
