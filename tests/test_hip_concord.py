"""mgv_concord_counts (csrc/concordance.hip) on the device against its restatement (tests/concord_ref.py, pinned on the CPU by
tests/test_concord_spec.py): every count is an integer and every comparison below is exact equality.  Then the surface:
ops.function_accuracy, Model.function_accuracy, the fixture the reference's get_function_acc produced
(tests/golden/g10_function_acc.npz), ops.pair_segments' refusals, Trainer --val_func_acc and feature_extract.py --function_acc."""
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import concord_ref as CR  # noqa: E402
from conftest import load_golden  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
NAN = float('nan')
GAPS = {1: (0.05,), 3: (0.0, 0.05, 7.0), 8: (0.0, 0.05, 0.1, 7.0, 0.15, 0.05, 0.3, 0.25)}     # 7.0: a gap no comparison reaches


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _T():
    from deepgate import ops
    assert ops.CONCORD_TILE == CR.TILE
    return ops.CONCORD_TILE


def _device_counts(gt, pred, seg, gaps, dev):
    from deepgate import ops
    out = ops.concord_counts(torch.as_tensor(np.asarray(gt, dtype=F32), device=dev), torch.as_tensor(np.asarray(pred, dtype=F32), device=dev),
                             None if seg is None else torch.as_tensor(np.asarray(seg), dtype=torch.int32, device=dev), gaps)
    assert out.dtype == torch.int64 and out.is_cuda
    return out.cpu().numpy()


def _check(gt, pred, seg, gaps, dev):
    got = _device_counts(gt, pred, seg, gaps, dev)
    want = CR.counts_numpy(gt, pred, seg, gaps)
    if seg is not None:
        want = want[:len(seg) - 1]
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    return got


# ------------------------------------------------------------------------------------------------ one segment
@pytest.mark.parametrize('B', [1, 3, 8])
def test_one_segment_at_every_size_around_the_tile(B):
    dev, T = _dev(), _T()
    for P in (0, 1, 2, 3, T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 5):
        gt, pred = CR.random_case(P, P + B)
        got = _check(gt, pred, None, GAPS[B], dev)
        assert got.shape == (1, B, 3)
        if P > 3:
            assert got[0, 0, 0] > 0 and got[0, 0, 2] > 0           # eligible comparisons and eligible prediction ties
        if B > 1:
            assert (got[0, GAPS[B].index(7.0)] == 0).all()


# ------------------------------------------------------------------------------------------------ several segments
def _ptr(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def test_segments_of_every_shape():
    dev, T = _dev(), _T()
    cases = {'mixed lengths': _ptr([0, 1, T + 1, 0, 2, 2 * T - 1]), '100 segments of 3 pairs': _ptr([3] * 100),
             'boundary on a tile edge': _ptr([T, T + 7]), 'boundary one row before the edge': _ptr([T - 1, T + 8]),
             'boundary one row behind the edge': _ptr([T + 1, T + 6]), 'an empty last segment': _ptr([T + 3, 40, 0])}
    for name, seg in cases.items():
        P = int(seg[-1])
        gt, pred = CR.random_case(P, len(name))
        for B in (1, 8):
            got = _check(gt, pred, seg, GAPS[B], dev)
            assert got[:, 0, 0].sum() > 0, name
    # no table is one explicit segment
    gt, pred = CR.random_case(2 * T + 9, 77)
    assert np.array_equal(_device_counts(gt, pred, None, GAPS[3], dev), _device_counts(gt, pred, [0, 2 * T + 9], GAPS[3], dev))
    # a table whose segments leave pairs out at both ends
    _check(gt, pred, [5, T - 2, T + 30], GAPS[3], dev)


# ------------------------------------------------------------------------------------------------ designed values
def test_designed_values():
    dev = _dev()
    from deepgate import ops
    at = F32(0.05)
    below = np.nextafter(at, F32(0))
    ramp = np.arange(40, dtype=F32)
    cases = {
        'equal gt': (np.full(40, 0.25, dtype=F32), ramp),
        'equal pred': (ramp * F32(0.1), np.full(40, 0.5, dtype=F32)),
        'exactly at the gap': (np.array([0, at, 0.5, 0.5 + 2 * at], dtype=F32), [0.0, 1.0, 2.0, 3.0]),
        'one ulp below the gap': (np.array([0, below, 0.5], dtype=F32), [0.0, 1.0, 2.0]),
        'NaN in gt': (np.array([0, NAN, 1, 2, NAN], dtype=F32), [0.0, 1.0, 2.0, 1.0, 0.0]),
        'NaN in pred': ([0.0, 1.0, 2.0, 3.0, 4.0], np.array([0, NAN, 2, 2, NAN], dtype=F32)),
        'infinities': (np.array([0, np.inf, -np.inf, np.inf, 1], dtype=F32), np.array([0, 1, np.inf, np.inf, -np.inf], dtype=F32)),
    }
    gaps = (0.0, 0.05)
    for name, (gt, pred) in cases.items():
        got = _check(gt, pred, None, gaps, dev)
        if name == 'equal gt':
            assert (got == 0).all()
        if name == 'equal pred':
            assert (got[0, :, 1] == 0).all() and (got[0, :, 2] == got[0, :, 0]).all() and got[0, 0, 0] == 40 * 39 // 2
        if name == 'exactly at the gap':
            assert got[0, 1, 0] == 6                               # (0, at) and (0.5, 0.5 + 2 at) included: >=
        if name == 'one ulp below the gap':
            assert got[0, 0, 0] == 3 and got[0, 1, 0] == 2
        if name == 'NaN in gt':
            assert got[0, 0].tolist() == [3, 2, 0]
        if name == 'NaN in pred':
            assert got[0, 0].tolist() == [10, 2, 1]                # (0, 2), (0, 3) concordant; (2, 3) tied; the NaN rows neither
    # nothing eligible: accuracy -1
    hf = torch.rand(6, 16, device=dev) + 0.1
    pairs = torch.tensor([[0, 1, 2, 3], [1, 2, 3, 4]], device=dev)
    acc, counts = ops.function_accuracy(hf, pairs, torch.full((4,), 0.3, device=dev))
    assert acc.dtype == torch.float64 and acc.tolist() == [[-1.0]] and counts.tolist() == [[[0, 0, 0]]]


def test_counts_past_32_bits_match_the_closed_form():
    dev = _dev()
    P = 70001
    gt = CR.ladder(P)
    for gaps, ks in (((2.0 ** -17,), (1,)), ((3 * 2.0 ** -17, 2.0 ** -17, 0.0, 1000 * 2.0 ** -17, 70000 * 2.0 ** -17), (3, 1, 1, 1000, 70000))):
        want = [CR.closed_form(P, k) for k in ks]
        assert want[1 if len(ks) > 1 else 0] > 2 ** 31
        same = _device_counts(gt, gt, None, gaps, dev)
        assert same[0].tolist() == [[w, w, 0] for w in want]
        flip = _device_counts(gt, -gt, None, gaps, dev)
        assert flip[0].tolist() == [[w, 0, 0] for w in want]


def test_out_is_overwritten_guards_stay_and_a_table_beyond_p_is_clamped():
    dev, T = _dev(), _T()
    from deepgate import _hip, metrics
    from deepgate._hip import ptr
    P = 2 * T + 11
    gt, pred = CR.random_case(P, 5)
    seg = np.array([0, 40, T + 3, P + 1000], dtype=np.int64)       # the last end lies beyond P: clamped, well defined by the contract
    want = CR.counts_numpy(gt, pred, seg, GAPS[3])
    assert np.array_equal(want, CR.counts_numpy(gt, pred, [0, 40, T + 3, P], GAPS[3]))
    g, p = torch.as_tensor(gt, device=dev), torch.as_tensor(pred, device=dev)
    sp = torch.as_tensor(seg, dtype=torch.int32, device=dev)
    n = 3 * 3 * 3
    hg = metrics._concord_gaps(GAPS[3])
    bufs = []
    for sentinel in (-7, 123456789012345):
        buf = torch.full((n + 64,), sentinel, dtype=torch.int64, device=dev)
        _hip.call('mgv_concord_counts', P, ptr(g), ptr(p), ptr(sp), 3, hg, 3, ptr(buf))
        torch.cuda.synchronize()
        assert (buf[n:] == sentinel).all()                         # the 64 guard entries behind out
        assert np.array_equal(buf[:n].cpu().numpy().reshape(3, 3, 3), want)
        bufs.append(buf[:n].clone())
    assert torch.equal(bufs[0], bufs[1])                           # the same bytes from call to call
    # P = 0 zeroes out and launches nothing
    buf = torch.full((3 + 64,), -7, dtype=torch.int64, device=dev)
    _hip.call('mgv_concord_counts', 0, None, None, None, 0, hg, 1, ptr(buf))
    torch.cuda.synchronize()
    assert buf[:3].tolist() == [0, 0, 0] and (buf[3:] == -7).all()


# ------------------------------------------------------------------------------------------------ through the surface
def _aig_model(dev, seed=5):
    import deepgate
    torch.manual_seed(seed)
    enc = deepgate.digae_layer.DirectMultiGCNEncoder(dim_feature=6, dim_hidden=64, s_rounds=2, t_rounds=2, layernorm=True)
    model = deepgate.dg_ae_model_aig.Model(struct_encoder=enc, dim_hidden=64).to(dev)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return model


def test_function_accuracy_of_ops_and_model_on_a_two_graph_batch():
    dev = _dev()
    import deepgate
    from deepgate import ops, synthetic as syn
    model = _aig_model(dev).eval()
    arrays = syn.collate([syn.make_graph('aig', 1024, 12, 5100 + i, n_inputs=64) for i in range(2)])
    batch = deepgate.CircuitBatch.from_arrays(arrays, device=dev)
    with torch.no_grad():
        _, hf = model(batch)
    pi, tt = batch['tt_pair_index'], batch['tt_sim']
    gaps = (0.05, 0.0, 0.2)
    pred = (1 - ops.sim_at(hf, pi)).cpu().numpy()
    assert pred.dtype == F32 and np.array_equal(pred, (1 - model.functional_similarity(hf, pi)).cpu().numpy())
    seg = ops.pair_segments(pi, batch.graph_ptr, cache=batch)
    assert seg.dtype == torch.int32 and seg.is_cuda and seg.numel() == 3 and int(seg[-1]) == pi.shape[1] and int(seg[1]) > 0
    assert ops.pair_segments(pi, batch.graph_ptr, cache=batch) is seg
    want = CR.counts_numpy(tt.cpu().numpy(), pred, seg.cpu().numpy(), gaps)
    assert want[:, 0, 0].min() > 100                               # both circuits have comparisons to order
    acc, counts = ops.function_accuracy(hf, pi, tt, graph_ptr=batch.graph_ptr, gaps=gaps, cache=batch)
    assert acc.is_cuda and acc.dtype == torch.float64 and acc.shape == (2, 3) and counts.shape == (2, 3, 3)
    assert np.array_equal(counts.cpu().numpy(), want)
    assert np.array_equal(acc.cpu().numpy(), CR.accuracy(want))
    macc, mcounts = model.function_accuracy(hf, pi, tt, graph_ptr=batch.graph_ptr, min_gap=list(gaps))
    assert torch.equal(macc, acc) and torch.equal(mcounts, counts)
    macc1, mcounts1 = model.function_accuracy(hf, pi, tt, graph_ptr=batch.graph_ptr)         # a float: the reference's MIN_GAP
    assert torch.equal(macc1, acc[:, :1]) and torch.equal(mcounts1, counts[:, :1])
    one, _ = model.function_accuracy(hf, pi, tt)                                             # no graph_ptr: one circuit of all pairs
    assert one.shape == (1, 1) and np.array_equal(one.cpu().numpy(), CR.accuracy(CR.counts_numpy(tt.cpu().numpy(), pred, None, (0.05,))))


def test_the_reference_fixture_is_reproduced_through_the_model():
    dev = _dev()
    z = load_golden('g10_function_acc')
    model = _aig_model(dev).eval()
    hf = torch.from_numpy(z['hf']).to(dev)
    pairs, tt = torch.from_numpy(z['pairs']).to(dev), torch.from_numpy(z['tt_dis']).to(dev)
    acc, counts = model.function_accuracy(hf, pairs, tt, graph_ptr=torch.from_numpy(z['graph_ptr']))
    assert np.array_equal(acc.cpu().numpy()[:, 0], z['acc']), (acc.tolist(), z['acc'].tolist())
    assert counts[6, 0].tolist() == [0, 0, 0] and int(counts[4, 0, 2]) >= 2


def test_pair_segments_refuses_crossing_and_ungrouped_pairs():
    dev = _dev()
    from deepgate import ops
    gp = torch.tensor([0, 10, 25], device=dev)
    ok = torch.tensor([[0, 3, 11, 24], [9, 4, 12, 10]], device=dev)
    assert ops.pair_segments(ok, gp).tolist() == [0, 2, 4]
    with pytest.raises(ValueError):
        ops.pair_segments(torch.tensor([[0, 3, 11], [9, 10, 12]], device=dev), gp)            # (3, 10) crosses circuits
    with pytest.raises(ValueError):
        ops.pair_segments(torch.tensor([[0, 11, 3], [9, 12, 4]], device=dev), gp)             # not grouped by circuit
    with pytest.raises(ValueError):
        ops.function_accuracy(torch.rand(25, 16, device=dev), torch.tensor([[0, 11, 3], [9, 12, 4]], device=dev),
                              torch.rand(3, device=dev), graph_ptr=gp)


LINE_TODAY = r'val\| Epoch: \d+/\d+ \|Recon: \d+\.\d{4} \|ACC: \d+\.\d{2} \|Prob: \d+\.\d{4} \|Func: \d+\.\d{4}\|Net: \d+\.\d{2}s'


@pytest.mark.parametrize('val_auc', [False, True])
def test_trainer_val_line_with_val_func_acc(tmp_path, val_auc):
    dev = _dev()
    import deepgate
    from deepgate import synthetic as syn
    model = _aig_model(dev)
    graphs = [syn.make_graph('aig', 512, 10, 7700 + i, n_inputs=32) for i in range(4)]
    args = types.SimpleNamespace(model='DG_AE', val_func_acc=True, **({'val_auc': True} if val_auc else {}))
    tr = deepgate.Trainer(args, model, training_id='v', save_dir=str(tmp_path), lr=1e-4, rc_prob_func_weight=[1.0, 4.0, 4.0],
                          device='cuda:0', batch_size=2, distributed=False)
    from deepgate.trainer import GraphLoader
    tr.train(1, graphs, GraphLoader(graphs, 2, shuffle=False))     # val batches in order: (0, 1), (2, 3), as recomputed below
    lines = open(tr.log_path).read().splitlines()
    val = [ln for ln in lines if ln.startswith('val|')]
    train = [ln for ln in lines if ln.startswith('train|')]
    assert len(val) == 1 and len(train) == 1
    fields = ['Epoch', 'Recon', 'ACC', 'Prob', 'Func', 'Net']
    assert re.findall(r'(\w+):', train[0]) == fields and re.fullmatch(LINE_TODAY.replace('val', 'train', 1), train[0])
    assert re.findall(r'(\w+):', val[0]) == fields + (['AUC', 'AP'] if val_auc else []) + ['FuncAcc']
    m = re.fullmatch(LINE_TODAY + (r' \|AUC: \d\.\d{4} \|AP: \d\.\d{4}' if val_auc else '') + r' \|FuncAcc: (\d\.\d{4})', val[0])
    assert m, val[0]
    assert 0.0 <= float(m.group(1)) <= 1.0
    # the column is the mean over the phase's circuits of concordant / eligible at gap 0.05, from the run's own counts
    model.eval()
    accs = []
    with torch.no_grad():
        for b0 in (0, 2):
            batch = deepgate.CircuitBatch.from_arrays(syn.collate(graphs[b0:b0 + 2]), device=dev)
            ls = tr.run_batch(batch, want_pred=False, want_func_acc=True)
            c = ls['func_counts'].cpu().numpy()
            assert c.shape == (2, 3) and (c[:, 0] > 0).all()
            accs += (c[:, 1] / c[:, 0]).tolist()
            assert 'func_counts' not in tr.run_batch(batch, want_pred=False)
    assert '%.4f' % (sum(accs) / len(accs)) == m.group(1)


def test_feature_extract_stores_the_accuracy_of_every_graph(tmp_path, monkeypatch, capsys):
    _dev()
    from conftest import PKG_PARENT
    monkeypatch.syspath_prepend(os.path.join(PKG_PARENT, 'examples'))
    import importlib
    fe = importlib.import_module('feature_extract')
    fe.main(['--type', 'aig', '--synthetic', '3', '--rounds', '2', '--batch_size', '2', '--out', str(tmp_path / 'emb.npz'),
             '--function_acc', '0.05,0.1'])
    text = capsys.readouterr().out
    z = np.load(tmp_path / 'emb.npz')
    names = sorted({k.split('/')[0] for k in z.files})
    assert len(names) == 3
    for name in names:
        acc, cnt = z[name + '/func_acc'], z[name + '/func_counts']
        assert acc.shape == (2,) and acc.dtype == np.float64 and cnt.shape == (2, 3) and cnt.dtype == np.int64
        assert (cnt[:, 0] > 0).all() and cnt[1, 0] <= cnt[0, 0] and np.array_equal(acc, cnt[:, 1] / cnt[:, 0])
        assert re.search(r'\[INFO\] %s: functional ordering accuracy \d\.\d{4} at gap 0\.05 ' % re.escape(name), text)
