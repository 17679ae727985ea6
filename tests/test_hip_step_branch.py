"""GPU tests of the training step's second-stream branch (Trainer.overlap): which launcher goes on which stream, that
the overlapped step computes what the one-stream step computes, and that no autograd node signals another through a module.
Through the public surface only (Trainer.overlap / run_batch / weighted_loss, Model.recon_loss, ops.FuncSweepFn / ReconLossFn)."""
import collections
import itertools
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H = 64
WEIGHTS = [1.0, 4.0, 4.0]
CASES = ('plain', 'hub', 'rounds2')      # 'hub': a primary input above GraphPlan.HEAVY_ROW consumers; 'rounds2': num_rounds = 2
GRAD_BOUND = {'plain': 0.0, 'hub': 0.0, 'rounds2': 4 * 3.603e-06}      # overlap on against off, per tensor (see the numbers test)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _batch(dev, hub):
    """Two AIG graphs of 304 nodes, without fixed negatives (the device sampler draws); hub: input 5 also drives 80 more gates."""
    import deepgate
    from deepgate import synthetic as syn
    graphs = [syn.make_graph('aig', 304, 8, 5100 + i, n_inputs=16) for i in range(2)]
    for g in graphs:
        del g['neg_edge_index']
    arrays = syn.collate(graphs)
    if hub:
        ei, n = arrays['edge_index'], arrays['num_nodes']
        have = set((ei[0] * n + ei[1]).tolist())
        gates = np.nonzero(arrays['forward_level'][:304] > 0)[0]
        dst = np.array([d for d in np.random.Generator(np.random.PCG64(4)).choice(gates, size=80, replace=False) if (5 * n + d) not in have])
        arrays['edge_index'] = np.concatenate([ei, np.stack([np.full(len(dst), 5, dtype=ei.dtype), dst.astype(ei.dtype)])], axis=1)
    return deepgate.CircuitBatch.from_arrays(arrays, device=dev)


_RUNS = {}


def _runs(case, monkeypatch):
    """One model and batch per case, stepped to the plan's steady state (packed rows come with its second step), then recorded:
    the step (run_batch, weighted_loss, backward) twice with overlap on and twice with it off, and the reconstruction branch alone
    (hs_decompose, sampler, loss; forward and backward) on the current stream.  Computed once, shared by the tests below."""
    if case in _RUNS:
        return _RUNS[case]
    dev = _dev()
    import deepgate
    from deepgate import _hip, sampling
    torch.manual_seed(9)
    enc = deepgate.digae_layer.DirectMultiGCNEncoder(dim_feature=6, dim_hidden=H, s_rounds=2, t_rounds=2, layernorm=True)
    model = deepgate.dg_ae_model_aig.Model(struct_encoder=enc, num_rounds=2 if case == 'rounds2' else 1, dim_hidden=H)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    model.to(dev).train()
    batch = _batch(dev, case == 'hub')
    tr = deepgate.Trainer(types.SimpleNamespace(model='DG_AE'), model, training_id='branch', save_dir='/tmp/mgv_test_exp', lr=1e-4,
                          rc_prob_func_weight=WEIGHTS, device='cuda:0', batch_size=2, distributed=False)
    record = []
    real = _hip.call

    def shim(name, *args):
        record.append((name, _hip.stream().value))
        return real(name, *args)
    monkeypatch.setattr(_hip, 'call', shim)

    def step(overlap):
        monkeypatch.setattr(sampling, '_CALLS', itertools.count())      # the sampled negatives repeat
        tr.overlap = overlap
        tr.optimizer.zero_grad()
        del record[:]
        ls = tr.run_batch(batch, want_pred=False)
        tr.weighted_loss(ls).backward()
        torch.cuda.synchronize()
        return {'launches': list(record),
                'losses': [ls[k].detach().clone() for k in ('recon_loss', 'prob_loss', 'func_loss')], 'confusion': ls['confusion'].clone(),
                'grads': {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}}

    step(True), step(True)
    out = {'on': [step(True), step(True)], 'off': [step(False), step(False)], 'main': _hip.stream().value}
    with torch.no_grad():
        hs, _ = model(batch)
    hs = hs.detach().requires_grad_(True)
    monkeypatch.setattr(sampling, '_CALLS', itertools.count())
    del record[:]
    loss = model.recon_loss(hs, batch.edge_index, None, want_pred=False, plan=batch._mgv_plan, expect_scale=WEIGHTS[0],
                            graph_ptr=batch.graph_ptr)[0]
    (WEIGHTS[0] * loss).backward()
    torch.cuda.synchronize()
    out['branch'] = [name for name, _ in record]
    if case == 'hub':
        assert batch._mgv_plan.heavy_segments(True) is not None
    _RUNS[case] = out
    return out


@pytest.mark.parametrize('case', CASES)
def test_the_second_stream_carries_the_reconstruction_branch_and_nothing_else(case, monkeypatch):
    """overlap on: the launchers on the second stream are, in order, those the reconstruction branch makes when it is driven alone
    (hs_decompose forward, sampler, one-walk loss with its heavy-list launches; mgv_rows_rescale_unless and the hs_decompose backward),
    every other launcher is on the main stream; overlap off: one stream; the same launchers either way."""
    r = _runs(case, monkeypatch)
    on, off, main = r['on'][0]['launches'], r['off'][0]['launches'], r['main']
    streams = {s for _, s in on}
    assert main in streams and len(streams) == 2, streams
    side = [name for name, s in on if s != main]
    assert side == r['branch']
    assert {'mgv_recon_step_csr', 'mgv_rows_rescale_unless'} <= set(side)
    assert ('mgv_recon_step_heavy_lists' in side) == (case == 'hub')
    names_on = collections.Counter(name for name, _ in on)
    assert names_on['mgv_func_sweep_fwd_x3'] == names_on['mgv_func_sweep_bwd_x3'] == (2 if case == 'rounds2' else 1)
    assert {s for _, s in off} == {main}
    assert names_on == collections.Counter(name for name, _ in off)
    assert r['on'][1]['launches'] == on and r['off'][1]['launches'] == off


@pytest.mark.parametrize('case', CASES)
def test_the_overlapped_step_computes_what_the_one_stream_step_computes(case, monkeypatch):
    """Losses and confusion counters: the same bits with overlap on and off (the same kernels on the same inputs), and from run to
    run.  Parameter gradients: the same bits from run to run of one setting.  Between the settings they differ only in where the
    gradients of hs's consumers meet (inside hs_decompose's input-gradient kernel, or in autograd's adds): with one round that is a
    sum of two terms either way and the bits agree (measured on these batches before the branch object existed: 0 of 56 tensors
    differ), with two rounds hs has three consumers, the sum is taken in another order and 30 of 58 tensors differed, by at most
    3.603e-06 of the tensor's largest entry (struct_encoder.target_conv.update.weight_ih_l0): GRAD_BOUND is 4 x that, per tensor."""
    r = _runs(case, monkeypatch)
    for a, b in ((r['on'][0], r['on'][1]), (r['off'][0], r['off'][1]), (r['on'][0], r['off'][0])):
        assert all(torch.equal(x, y) for x, y in zip(a['losses'], b['losses']))
        assert torch.equal(a['confusion'], b['confusion']) and int(a['confusion'].sum()) > 0
    for setting in ('on', 'off'):
        a, b = r[setting]
        assert a['grads'].keys() == b['grads'].keys()
        diff = [k for k in a['grads'] if not torch.equal(a['grads'][k], b['grads'][k])]
        assert not diff, (setting, diff)
    a, b = r['on'][0]['grads'], r['off'][0]['grads']
    assert a.keys() == b.keys()
    rel = {k: float((a[k] - b[k]).abs().max()) / max(float(b[k].abs().max()), 1e-30) for k in a}
    worst = max(rel, key=rel.get)
    print('overlap on against off, %s: largest relative gradient difference %.3e (%s), %d of %d tensors differ'
          % (case, rel[worst], worst, sum(v > 0 for v in rel.values()), len(rel)))
    assert rel[worst] <= GRAD_BOUND[case], (worst, rel[worst])


def test_a_loss_backward_waits_for_no_event_of_an_earlier_sweep_backward(monkeypatch):
    """ops.FuncSweepFn forward and backward alone, then, in a fresh graph on the same stream, ops.ReconLossFn forward and backward
    alone: the second backward enqueues no event wait (the sweep backward leaves no signal behind for whichever loss runs next)."""
    dev = _dev()
    import deepgate
    from deepgate import ops
    batch = _batch(dev, False)
    plan = deepgate.data.plan_of(batch, [gid for _, gid in deepgate.dg_ae_model_aig.Model.GATES])
    N, T = plan.N, plan.num_slots
    g = torch.Generator().manual_seed(2)
    leaf = lambda *shape: (torch.randn(*shape, generator=g) * 0.2).to(dev).requires_grad_(True)       # noqa: E731
    hf = ops.FuncSweepFn.apply(plan, leaf(N, H), leaf(T, 2 * H), leaf(T, 3 * H, 2 * H), leaf(T, 3 * H), leaf(T, 3 * H), leaf(T, 3 * H))
    hf.backward(torch.randn(N, H, generator=g).to(dev))
    torch.cuda.synchronize()
    st = leaf(N, 2 * H)
    neg = torch.randint(0, N, (2, 500), generator=g).to(dev)
    loss = ops.ReconLossFn.apply(st, batch.edge_index, neg, False)[0]
    waits = []
    real = torch.cuda.Stream.wait_event
    monkeypatch.setattr(torch.cuda.Stream, 'wait_event', lambda self, event: (waits.append(event), real(self, event))[1])
    loss.backward()
    torch.cuda.synchronize()
    assert st.grad is not None and len(waits) == 0, waits
