"""Link-prediction ROC-AUC / average precision ranked on the device (csrc/link_metrics.hip) against the float64 restatement
(tests/link_metrics_ref.py), the decoder's own scores, the values the reference's DirectedGVAE.test produced
(tests/golden/g8_linkpred.npz) and through the public surface (DirectedGVAE.test, Model.link_metrics, recon_loss(want_rank=True),
Trainer.run_batch / --val_auc)."""
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden  # noqa: E402
from link_metrics_ref import rank_stats  # noqa: E402

pytestmark = pytest.mark.gpu

# |device - reference| of (AUC, AP) on the fixture's cases `plain` and `ties`: the device ranks its own fp32 scores (v_exp / v_rcp
# sigmoid, DPP dot product), the reference torch's CPU fp32 scores; the two orders differ only where two scores are nearly equal.
# Measured on the MI355X:   plain  AUC 0 (bit-equal)   AP 1.1e-16        ties  AUC 1.1e-16   AP 5.456e-08
# The constant is four times the larger measured difference of the two cases (the margin covers the box-to-box variation this
# project sees in fp32 sums).  For scale: fp32 against float64 scores on the CPU move AUC by 9.5e-8 and AP by 4.2e-8 at this size.
FIXTURE_TOL = 4 * 5.456e-08


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _check(s, t, pos, neg, st_layout=False):
    """Device ranking against the restatement ON THE DEVICE'S OWN SCORES: integers exactly, AUC to one double rounding, AP to the
    bound of two summation orders of the same n non-negative double terms (each within n * 2^-53 of the exact sum, relative)."""
    from deepgate import ops
    P, Q = pos.shape[1], neg.shape[1]
    n = P + Q
    if st_layout:
        metrics, status, scores, counts = ops.link_auc_ap(torch.cat([s, t], dim=1), None, pos, neg, return_scores=True)
    else:
        metrics, status, scores, counts = ops.link_auc_ap(s, t, pos, neg, return_scores=True)
    assert metrics.dtype == torch.float64 and metrics.shape == (2,) and metrics.is_cuda
    r = rank_stats(scores.cpu().numpy(), P)
    got = [int(v) for v in counts.tolist()]
    auc, ap = metrics.tolist()
    print('n=%d U2=%d groups=%d  AUC %.17g (ref %.17g)  AP %.17g (ref %.17g, diff %.3g)' % (n, got[0], got[3], auc, r['auc'], ap, r['ap'], abs(ap - r['ap'])))
    assert int(status.item()) == 0
    assert got == [r['U2'], r['P'], r['Q'], r['groups']]
    assert abs(auc - r['auc']) <= 1e-15
    assert abs(ap - r['ap']) <= n * 2.0 ** -52
    return r, scores


def _node_scores(logits, dev, H=16):
    """s, t [N, H] whose pair (u, v) scores sigmoid(logits[u]) for every v: exact control over ties and extremes."""
    N = len(logits)
    s = torch.zeros(N, H, device=dev)
    s[:, 0] = torch.as_tensor(logits, dtype=torch.float32, device=dev)
    t = torch.zeros(N, H, device=dev)
    t[:, 0] = 1.0
    return s, t


def _pairs_from(nodes, dev, N):
    src = torch.as_tensor(nodes, dtype=torch.int64, device=dev)
    return torch.stack([src, (src * 7 + 3) % N])


@pytest.mark.parametrize('n', [2, 3, 63, 64, 65, 4097])
@pytest.mark.parametrize('H', [16, 64])
def test_small_sizes_match_the_restatement_exactly(n, H):
    dev = _dev()
    g = torch.Generator().manual_seed(100 * n + H)
    N = 24                                              # 576 distinct pairs: natural ties from n = 4097 on
    s, t = (0.3 * torch.randn(N, H, generator=g)).to(dev), (0.3 * torch.randn(N, H, generator=g)).to(dev)
    P = max(n // 2, 1)
    pairs = torch.randint(0, N, (2, n), generator=g).to(dev)
    _check(s, t, pairs[:, :P], pairs[:, P:], st_layout=(H == 64))


@pytest.mark.parametrize('case', ['plain', 'ties', 'one'])
def test_fixture_cases_match_the_restatement_exactly(case):
    dev = _dev()
    z = load_golden('g8_linkpred')
    s, t = torch.from_numpy(z[case + '_s']).to(dev), torch.from_numpy(z[case + '_t']).to(dev)
    r, _ = _check(s, t, torch.from_numpy(z[case + '_pos']).to(dev), torch.from_numpy(z[case + '_neg']).to(dev))
    if case == 'one':
        assert r['groups'] == 1
    if case == 'ties':
        assert r['groups'] < 8256 - 1000


def test_separated_classes_give_the_extreme_values():
    dev = _dev()
    N = 512
    logits = np.concatenate([np.linspace(0.5, 3.0, N // 2), np.linspace(-3.0, -0.5, N // 2)])
    s, t = _node_scores(logits, dev)
    hi, lo = _pairs_from(np.arange(3000) % (N // 2), dev, N), _pairs_from(N // 2 + np.arange(5000) % (N // 2), dev, N)
    r, _ = _check(s, t, hi, lo)                         # every positive above every negative
    assert r['auc'] == 1.0 and r['ap'] == 1.0
    from deepgate import ops
    m, _ = ops.link_auc_ap(s, t, hi, lo)
    assert m.tolist() == [1.0, 1.0]
    r, _ = _check(s, t, lo, hi)                         # every positive below every negative
    assert r['auc'] == 0.0
    m, _ = ops.link_auc_ap(s, t, lo, hi)
    assert m[0].item() == 0.0


def test_one_tie_group_of_2_to_the_20():
    dev = _dev()
    n, P = 1 << 20, (1 << 19) + 3
    s, t = _node_scores(np.zeros(64), dev)
    nodes = np.arange(n) % 64
    r, scores = _check(s, t, _pairs_from(nodes[:P], dev, 64), _pairs_from(nodes[P:], dev, 64))
    assert r['groups'] == 1 and bool((scores == 0.5).all())
    from deepgate import ops
    m, _ = ops.link_auc_ap(s, t, _pairs_from(nodes[:P], dev, 64), _pairs_from(nodes[P:], dev, 64))
    assert m[0].item() == 0.5 and abs(m[1].item() - P / n) <= 1e-15


def test_zero_one_and_tiny_scores():
    """Logits chosen so that the sigmoid gives exactly 0.0f and 1.0f (many pairs each: long tie groups at both ends) and the smallest
    values the device's exp / rcp produce on the way there (denormals where the hardware keeps them)."""
    dev = _dev()
    logits = np.concatenate([[-200.0, -120.0, 30.0, 40.0, 0.0], np.linspace(-104.0, -85.0, 59)])
    s, t = _node_scores(logits, dev)
    N = len(logits)
    g = np.random.default_rng(5)
    nodes = g.integers(0, N, 50000)
    r, scores = _check(s, t, _pairs_from(nodes[:21000], dev, N), _pairs_from(nodes[21000:], dev, N))
    sc = scores.cpu().numpy()
    assert (sc == 0.0).sum() > 1000 and (sc == 1.0).sum() > 1000
    print('distinct scores %d, smallest positive %.3g' % (r['groups'], sc[sc > 0].min()))


def _rank_abi(skeys, order, P):
    """mgv_link_rank alone, on hand-built sorted keys and permutation."""
    from deepgate import _hip
    from deepgate._hip import ptr
    n = skeys.numel()
    rec = torch.zeros(8, dtype=torch.float64, device=skeys.device)
    w = _hip.call_value('mgv_link_rank_work_ints', n)
    assert w > 0
    work = torch.empty(w + 2, dtype=torch.int32, device=skeys.device)
    _hip.call('mgv_link_rank', n, P, ptr(skeys), ptr(order), ptr(rec), ptr(work), w)
    return rec


def test_alternating_labels_inside_long_tie_groups():
    """The radix sort is stable, so behind it a tie group holds its positives first; the rank pass must not depend on that.  Fed
    directly: tie groups whose lengths straddle the 2048-element tiles (1, 2, 2047, 2048, 2049, 300,000, ...), labels alternating
    inside every group.  Expected values: the restatement on scores laid out so that element order[i] has the i-th sorted score."""
    dev = _dev()
    rng = np.random.default_rng(11)
    runs = [1, 2, 7, 2047, 2048, 2049, 1, 5000, 300000, 3, 4096, 1, 1, 6143, 2, 100001, 2048, 2048, 1]
    runs += list(rng.integers(1, 50, 2000)) + [70000, 1]
    n = int(sum(runs))
    gid = np.repeat(np.arange(len(runs)), runs)                       # sorted position -> tie group, highest score first
    score = (1.0 - (gid + 1) / (len(runs) + 2)).astype(np.float32)    # strictly decreasing in the group index
    assert len(np.unique(score)) == len(runs)
    label = (np.arange(n) % 2 == 0)                                   # alternating through the sorted array
    P = int(label.sum())
    order = np.empty(n, dtype=np.int32)
    order[label] = rng.permutation(P)
    order[~label] = P + rng.permutation(n - P)
    u = score.view(np.uint32)
    skey = ~(u | np.uint32(0x80000000))                               # the kernel's key of a non-negative score
    assert (np.diff(skey.astype(np.int64)) >= 0).all()
    rec = _rank_abi(torch.from_numpy(skey.view(np.int32)).to(dev), torch.from_numpy(order).to(dev), P)
    laid = np.empty(n, dtype=np.float32)
    laid[order] = score
    r = rank_stats(laid, P)
    words = rec.view(torch.int64).tolist()
    auc, ap = rec[:2].tolist()
    print('n=%d groups=%d AUC %.17g AP %.17g (diff %.3g)' % (n, words[5], auc, ap, abs(ap - r['ap'])))
    assert words[2:6] == [r['U2'], r['P'], r['Q'], r['groups']] and r['groups'] == len(runs)
    assert abs(auc - r['auc']) <= 1e-15 and abs(ap - r['ap']) <= n * 2.0 ** -52
    assert torch.equal(rec, _rank_abi(torch.from_numpy(skey.view(np.int32)).to(dev), torch.from_numpy(order).to(dev), P))


def _baseline_graph(dev):
    from deepgate import synthetic as syn
    from deepgate.sampling import negative_sampling
    g = syn.make_graph('aig', 65536, 120, 2000, n_inputs=4096)
    pos = torch.from_numpy(np.ascontiguousarray(g['edge_index'])).long().to(dev)
    if pos.shape[0] != 2:
        pos = pos.t().contiguous()
    N = int(g['x'].shape[0]) if 'x' in g else 65536
    gen = torch.Generator().manual_seed(9)
    s, t = (0.3 * torch.randn(N, 64, generator=gen)).to(dev), (0.3 * torch.randn(N, 64, generator=gen)).to(dev)
    return s, t, pos, negative_sampling(pos, N), N


def test_one_baseline_graph_and_2_to_the_24_pairs_over_it():
    dev = _dev()
    s, t, pos, neg, N = _baseline_graph(dev)
    assert pos.shape[1] > 90000 and neg.shape[1] > 150000
    _check(s, t, pos, neg, st_layout=True)
    g = torch.Generator(device=dev).manual_seed(21)
    n, P = 1 << 24, 6000000
    pairs = torch.randint(0, N, (2, n), generator=g, device=dev)
    _check(s, t, pairs[:, :P].contiguous(), pairs[:, P:].contiguous())


def test_ranked_scores_are_the_decoders_bit_for_bit():
    """What is ranked is what DirectedInnerProductDecoder.forward(..., sigmoid=True) returns for the same pairs, in both layouts."""
    dev = _dev()
    from deepgate import ops
    from deepgate.digae_layer import DirectedInnerProductDecoder
    s, t, pos, neg, _ = _baseline_graph(dev)
    dec = DirectedInnerProductDecoder()(s, t, torch.cat([pos, neg], dim=1), sigmoid=True)
    for args in ((s, t), (torch.cat([s, t], dim=1), None)):
        _, _, scores, _ = ops.link_auc_ap(args[0], args[1], pos, neg, return_scores=True)
        assert torch.equal(scores, dec)


@pytest.mark.parametrize('case', ['plain', 'ties', 'one'])
def test_directed_gvae_test_against_the_reference_values(case):
    dev = _dev()
    from deepgate import digvae_model
    z = load_golden('g8_linkpred')
    model = digvae_model.DirectedGVAE(torch.nn.Identity(), 64)
    out = model.test(torch.from_numpy(z[case + '_s']).to(dev), torch.from_numpy(z[case + '_t']).to(dev),
                     torch.from_numpy(z[case + '_pos']).to(dev), torch.from_numpy(z[case + '_neg']).to(dev))
    assert isinstance(out, tuple) and len(out) == 2 and all(type(v) is float for v in out)
    auc, ap = out
    d_auc, d_ap = abs(auc - float(z[case + '_auc'])), abs(ap - float(z[case + '_ap']))
    print('%s: AUC %.17g (reference %.17g, diff %.3g)  AP %.17g (reference %.17g, diff %.3g)'
          % (case, auc, float(z[case + '_auc']), d_auc, ap, float(z[case + '_ap']), d_ap))
    if case == 'one':
        assert auc == 0.5 and abs(ap - 4000 / 8256) <= 1e-15
    else:
        assert d_auc <= FIXTURE_TOL and d_ap <= FIXTURE_TOL


def test_nan_score_raises_value_error_and_calls_repeat_bit_for_bit():
    dev = _dev()
    from deepgate import digvae_model, ops
    z = load_golden('g8_linkpred')
    s, t = torch.from_numpy(z['plain_s']).to(dev), torch.from_numpy(z['plain_t']).to(dev)
    pos, neg = torch.from_numpy(z['plain_pos']).to(dev), torch.from_numpy(z['plain_neg']).to(dev)
    a, b = ops.link_record(s, t, pos, neg), ops.link_record(s, t, pos, neg)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    model = digvae_model.DirectedGVAE(torch.nn.Identity(), 64)
    assert model.test(s, t, pos, neg) == tuple(a[:2].tolist())
    bad = s.clone()
    bad[int(pos[0, 0]), 3] = float('nan')
    _, status = ops.link_auc_ap(bad, t, pos, neg)
    assert int(status.item()) > 0
    with pytest.raises(ValueError):
        model.test(bad, t, pos, neg)


def _aig_model(dev, seed=5):
    import deepgate
    torch.manual_seed(seed)
    enc = deepgate.digae_layer.DirectMultiGCNEncoder(dim_feature=6, dim_hidden=64, s_rounds=2, t_rounds=2, layernorm=True)
    model = deepgate.dg_ae_model_aig.Model(struct_encoder=enc, dim_hidden=64).to(dev)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return model


def _batch(dev, n=3, nodes=1024, fixed_neg=True):
    import deepgate
    from deepgate import synthetic as syn
    arrays = syn.collate([syn.make_graph('aig', nodes, 12, 4400 + i, n_inputs=64) for i in range(n)])
    batch = deepgate.CircuitBatch.from_arrays(arrays, device=dev)
    if fixed_neg:
        N, E = arrays['num_nodes'], arrays['edge_index'].shape[1]
        g = torch.Generator().manual_seed(3)
        batch.neg_edge_index = torch.stack([torch.randint(0, N, (E + N,), generator=g), torch.randint(0, N, (E + N,), generator=g)]).to(dev)
    return batch


def test_model_link_metrics_is_the_op_on_hs_decompose():
    dev = _dev()
    from deepgate import ops
    model = _aig_model(dev).eval()
    batch = _batch(dev)
    with torch.no_grad():
        hs, _ = model(batch)
        rec = model.link_metrics(hs, batch.edge_index, batch.neg_edge_index)
        st = ops.linear(hs, model.hs_decompose.weight, model.hs_decompose.bias)
        direct = ops.link_record(st, None, batch.edge_index, batch.neg_edge_index)
        assert torch.equal(rec.view(torch.int64), direct.view(torch.int64))
        m, status = ops.link_auc_ap(st, None, batch.edge_index, batch.neg_edge_index)
        assert torch.equal(m, rec[:2]) and int(status.item()) == 0
        # negatives drawn like recon_loss draws them when none are given: as many as edges (without self loops) plus nodes
        drawn = model.link_metrics(hs, batch.edge_index, plan=getattr(batch, '_mgv_plan', None))
    words = drawn.view(torch.int64).tolist()
    assert words[3] == batch.edge_index.shape[1] and words[4] >= hs.shape[0] and words[6] == 0
    assert 0.0 <= drawn[0].item() <= 1.0 and 0.0 < drawn[1].item() <= 1.0


def test_want_rank_ranks_the_losss_own_pairs_and_leaves_the_step_bit_identical(tmp_path):
    dev = _dev()
    import deepgate
    from deepgate import ops
    model = _aig_model(dev).train()
    batch = _batch(dev)
    tr = deepgate.Trainer(types.SimpleNamespace(model='DG_AE'), model, training_id='rank', save_dir=str(tmp_path), lr=1e-4,
                          rc_prob_func_weight=[1.0, 4.0, 4.0], device='cuda:0', batch_size=3, distributed=False)
    runs = []
    for want_rank in (False, True, False):
        tr.optimizer.zero_grad()
        ls = tr.run_batch(batch, want_pred=False, **({'want_rank': True} if want_rank else {}))
        tr.weighted_loss(ls).backward()
        torch.cuda.synchronize()
        assert ('link_metrics' in ls) == want_rank
        assert (model.last_link_metrics is not None) == want_rank
        runs.append((ls, {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}))
    for ls, grads in runs[1:]:
        for k in ('recon_loss', 'prob_loss', 'func_loss', 'confusion'):
            assert torch.equal(ls[k], runs[0][0][k]), k
        assert [k for k in grads if not torch.equal(grads[k], runs[0][1][k])] == []
    # the record is the ranking of the loss's own pairs: the batch's edges against the fixed negatives, on st = hs_decompose(hs)
    with torch.no_grad():
        hs, _ = model(batch)
        st = ops.linear(hs, model.hs_decompose.weight, model.hs_decompose.bias)
        direct = ops.link_record(st, None, batch.edge_index, batch.neg_edge_index)
    rec = runs[1][0]['link_metrics']
    assert torch.equal(rec.view(torch.int64), direct.view(torch.int64))
    # the model's own entry point without the Trainer
    hs2 = hs.clone().requires_grad_(True)
    model.recon_loss(hs2, batch.edge_index, batch.neg_edge_index, want_pred=False, want_rank=True)
    assert torch.equal(model.last_link_metrics.view(torch.int64), direct.view(torch.int64))
    model.recon_loss(hs2, batch.edge_index, batch.neg_edge_index, want_pred=False)
    assert model.last_link_metrics is None


LINE_TODAY = r'val\| Epoch: \d+/\d+ \|Recon: \d+\.\d{4} \|ACC: \d+\.\d{2} \|Prob: \d+\.\d{4} \|Func: \d+\.\d{4}\|Net: \d+\.\d{2}s'


@pytest.mark.parametrize('val_auc', [False, True])
def test_trainer_val_line_with_and_without_val_auc(tmp_path, val_auc):
    dev = _dev()
    import deepgate
    from deepgate import synthetic as syn
    model = _aig_model(dev)
    graphs = [syn.make_graph('aig', 512, 10, 7700 + i, n_inputs=32) for i in range(4)]
    args = types.SimpleNamespace(model='DG_AE', val_auc=True) if val_auc else types.SimpleNamespace(model='DG_AE')
    tr = deepgate.Trainer(args, model, training_id='v', save_dir=str(tmp_path), lr=1e-4, rc_prob_func_weight=[1.0, 4.0, 4.0],
                          device='cuda:0', batch_size=2, distributed=False)
    tr.train(1, graphs, graphs)
    lines = open(tr.log_path).read().splitlines()
    val = [ln for ln in lines if ln.startswith('val|')]
    train = [ln for ln in lines if ln.startswith('train|')]
    assert len(val) == 1 and len(train) == 1
    fields = ['Epoch', 'Recon', 'ACC', 'Prob', 'Func', 'Net']          # the reference's phase line (trainer.py:259-262)
    assert re.findall(r'(\w+):', train[0]) == fields                      # the train line never changes
    if val_auc:
        assert re.findall(r'(\w+):', val[0]) == fields + ['AUC', 'AP']
        m = re.fullmatch(LINE_TODAY + r' \|AUC: (\d\.\d{4}) \|AP: (\d\.\d{4})', val[0])
        assert m, val[0]
        assert 0.0 <= float(m.group(1)) <= 1.0 and 0.0 < float(m.group(2)) <= 1.0
    else:
        assert re.findall(r'(\w+):', val[0]) == fields
        assert re.fullmatch(LINE_TODAY, val[0]), val[0]


def test_train_entry_with_val_auc_and_feature_extract_with_link_metrics(tmp_path, monkeypatch, capsys):
    """`python train.py ... --val_auc` logs the two columns on every val line of its three stages; the example script prints the
    checkpoint's AUC / AP behind --link_metrics."""
    _dev()
    from conftest import PKG_PARENT
    monkeypatch.syspath_prepend(PKG_PARENT)
    monkeypatch.syspath_prepend(os.path.join(PKG_PARENT, 'examples'))
    import importlib
    train = importlib.import_module('train')
    train.main(['--exp_id', 'e', '--model', 'DG_AE', '--type', 'aig', '--layernorm', '--batch_size', '2', '--synthetic', '20',
                '--synthetic_nodes', '256', '--synthetic_levels', '8', '--stage_epochs', '1', '1', '1', '--s_rounds', '2', '--t_rounds', '2',
                '--save_dir', str(tmp_path), '--val_auc'])         # 18 training graphs, 2 validation graphs = one val batch per epoch
    log = [f for f in os.listdir(tmp_path / 'e') if f.startswith('log-')]
    lines = open(tmp_path / 'e' / log[0]).read().splitlines()
    val = [ln for ln in lines if ln.startswith('val|')]
    assert len(val) == 3 and all(re.fullmatch(LINE_TODAY + r' \|AUC: \d\.\d{4} \|AP: \d\.\d{4}', ln) for ln in val), val
    assert all(re.fullmatch(LINE_TODAY.replace('val', 'train', 1), ln) for ln in lines if ln.startswith('train|'))
    fe = importlib.import_module('feature_extract')
    capsys.readouterr()
    fe.main(['--type', 'aig', '--synthetic', '3', '--checkpoint', str(tmp_path / 'e' / 'stage_3.pth'), '--rounds', '2', '--batch_size', '2',
             '--out', str(tmp_path / 'emb.npz'), '--link_metrics'])
    m = re.search(r'link prediction over 2 batches: AUC (\d\.\d{4}), AP (\d\.\d{4})', capsys.readouterr().out)
    assert m and 0.0 <= float(m.group(1)) <= 1.0 and 0.0 < float(m.group(2)) <= 1.0
