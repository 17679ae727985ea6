"""mgv_fanin_decode (csrc/pair_scores.hip) and mgv_fanin_recovery (csrc/fanin_recovery.hip) through the C ABI and through the surface
(ops.fanin_decode / fanin_edges / fanin_recovery, Model.decode_circuit / circuit_recovery, DirectedGAE, feature_extract.py
--decode_circuit, train.py --val_recovery), against tests/fanin_decode_ref.py (pinned on the CPU by tests/test_fanin_decode_spec.py,
which also asserts the properties of the case builders used here, shows the planted defects to change the result, and shows the
orthonormal design to be recovered exactly by the restatement).

Exact: idx and n_cand equal the restatement run on the device's own dense scores (mgv_pair_scores_fwd, sigmoid = 0, operands swapped)
as integers and score bit for bit, also against mgv_pair_scores_at; with and without tile_min the same bytes; two calls the same bytes.
Conventions of tests/test_hip_pair_scores.py: operands are column slices of wider matrices whose foreign columns hold NaN; every output
has 64 guard rows behind it and is filled before the call.  Every check prints one line `FANIN <what> | figures`."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fanin_decode_ref as FR  # noqa: E402
import test_hip_pair_scores as TP  # noqa: E402  (Out, the operand slices and the launcher helpers of the pair-score tests)
from conftest import PKG_PARENT  # noqa: E402

pytestmark = pytest.mark.gpu

F32, I32, I64 = torch.float32, torch.int32, torch.int64
HS = (16, 32, 64, 128)
MGV_EINVAL, MGV_EUNSUPPORTED = -1, -2
Out, _dev, _ptr, _rc, _call, _bits, _slice = TP.Out, TP._dev, TP._ptr, TP._rc, TP._call, TP._bits, TP._slice


class Decode:
    """One mgv_fanin_decode through the raw ABI on strided operands; every output an Out of the test's own."""

    def __init__(self, dev, c, skip, K=None, H=None):
        N, K = c['N'], c['K'] if K is None else K
        self.tv, ldt = _slice(c['t'], dev)
        self.sv, lds = _slice(c['s'], dev)
        gp = c['graph_ptr']
        self.gpd = None if gp is None else torch.tensor(gp, dtype=I32, device=dev)
        self.key = torch.from_numpy(c['key']).to(dev)
        self.want = torch.from_numpy(c['want']).to(dev)
        self.tile_min = Out((N + 63) // 64, 1, dev, dtype=I32) if skip else None
        self.idx, self.score, self.n_cand = Out(N, max(K, 1), dev, dtype=I32), Out(N, max(K, 1), dev), Out(N, 1, dev, dtype=I32)
        self.args = lambda: (c['H'] if H is None else H, N, _ptr(self.tv), ldt, _ptr(self.sv), lds, _ptr(self.gpd),
                             0 if gp is None else len(gp) - 1, _ptr(self.key), _ptr(self.want), K,
                             None if self.tile_min is None else _ptr(self.tile_min.v), _ptr(self.idx.v), _ptr(self.score.v), _ptr(self.n_cand.v))

    def run(self):
        _call('mgv_fanin_decode', *self.args())
        return self

    def rc(self):
        return _rc('mgv_fanin_decode', *self.args())

    def result(self):
        return self.idx.v.cpu().numpy(), self.score.v.cpu().numpy(), self.n_cand.v.flatten().cpu().numpy()

    def outs(self):
        return [o for o in (self.idx, self.score, self.n_cand, self.tile_min) if o is not None]

    def intact(self):
        return all(o.intact() for o in self.outs())

    def untouched(self):
        return all(o.untouched() for o in self.outs())

    def bytes(self):
        return [_bits(o.parent) for o in (self.idx, self.score, self.n_cand)]


def _dense(dev, c):
    """scores[v][u] on the device: mgv_pair_scores_fwd with the operands swapped, raw."""
    return TP._fwd(dev, c['t'], c['s'], 0)[0].v.cpu().numpy()


def _check(dev, c, tag):
    """Both forms of the walk against the restatement on the device's dense scores -> list of complaints."""
    bad = []
    dense = _dense(dev, c)
    ref = FR.decode_ref(dense, c['key'], c['want'], c['K'], c['graph_ptr'])
    plain, skip = Decode(dev, c, False).run(), Decode(dev, c, True).run()
    for name, d in (('tile_min NULL', plain), ('tile_min given', skip)):
        if not FR.same_decode(d.result(), ref):
            got = d.result()
            rows = np.nonzero((got[0] != ref[0]).any(1) | (got[2] != ref[2]) | (got[1].view(np.int32) != ref[1].view(np.int32)).any(1))[0]
            bad.append('%s %s: rows %s differ from the restatement' % (tag, name, rows[:8].tolist()))
        if not d.intact():
            bad.append('%s %s: guard rows changed' % (tag, name))
    if not all(torch.equal(a, b) for a, b in zip(plain.bytes(), skip.bytes())):
        bad.append('%s: the skip changes the output' % tag)
    first = skip.bytes()
    for o in (skip.idx, skip.n_cand):
        o.parent.fill_(-77)
    skip.score.parent.fill_(TP.NAN)
    skip.run()
    if not all(torch.equal(a, b) for a, b in zip(first, skip.bytes())):
        bad.append('%s: a second call gives other bytes' % tag)
    # the listed scores are the bits mgv_pair_scores_at reports for (u, v)
    idx = torch.from_numpy(ref[0])
    keep = idx >= 0
    if bool(keep.any()):
        src = idx[keep].to(I64).to(dev)
        dst = torch.arange(c['N']).repeat_interleave(idx.shape[1]).view(idx.shape)[keep].to(dev)
        at = Out(src.numel(), 1, dev)
        _call('mgv_pair_scores_at', c['H'], src.numel(), _ptr(skip.sv), skip.sv.stride(0), _ptr(skip.tv), skip.tv.stride(0), _ptr(src), _ptr(dst), 0,
              _ptr(at.v))
        if not torch.equal(_bits(at.v.flatten()), _bits(skip.score.v.cpu()[keep])):
            bad.append('%s: a score is not the bits of mgv_pair_scores_at' % tag)
    return bad, ref


# ------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize('H', HS)
def test_decode_equals_the_restatement_on_every_designed_case(H):
    """N in {1, 2, 63, 64, 65, 129, 200} as one graph; graphs of (1, 5, 58, 64, 1, 71) nodes and the same 200 nodes as one graph with keys
    ascending, descending, levels 0 .. 5 and all equal, K in {1, 2, 3, 8}, want mixed over 0 .. K with a negative one and one above K,
    equal embedding rows, a NaN column row and a NaN target row (tests/fanin_decode_ref.py decode_case)."""
    dev = _dev()
    bad, listed, short = [], 0, 0
    for name, kw in FR.designed_cases(H):
        c = FR.decode_case(**kw)
        b, ref = _check(dev, c, 'H=%d %s' % (H, name))
        bad += b
        listed += int((ref[0] >= 0).sum())
        short += int((ref[2] < c['want']).sum())
        if c['keys'] == 'equal':
            d = Decode(dev, c, True).run()
            assert bool((d.idx.v == -1).all()) and bool((d.n_cand.v == 0).all()) and bool(torch.isinf(d.score.v).all())
    print('FANIN exact H=%d | %d cases, %d fan-ins listed, %d rows short of their want | %d complaints'
          % (H, len(FR.designed_cases(H)), listed, short, len(bad)))
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('H', HS)
def test_decode_on_a_long_graph_where_tiles_are_skipped(H):
    """One graph of 64 * 40 + 3 nodes, keys ascending with the id: 41 column tiles, of which row tile b walks b + 1 with tile_min;
    the rows of tile 7 want nothing and walk nothing."""
    dev = _dev()
    c = FR.long_case(H)
    bad, ref = _check(dev, c, 'H=%d long' % H)
    assert (ref[2][7 * 64:8 * 64] == 0).all() and (ref[0][7 * 64:8 * 64] == -1).all()
    print('FANIN long H=%d | %d fan-ins listed | %d complaints' % (H, int((ref[0] >= 0).sum()), len(bad)))
    assert not bad, '\n'.join(bad)


def test_shuffled_keys_and_keys_of_any_sign():
    """Keys far apart and of both signs, shuffled over the ids of three graphs: a skip can only drop tiles that hold nobody's candidate."""
    dev = _dev()
    c = FR.decode_case(H=32, sizes=(130, 7, 190), keys='asc', K=3, seed=5)
    rng = np.random.Generator(np.random.PCG64(5))
    c['key'] = (rng.permutation(c['N']).astype(np.int64) * 6000000 - 2 ** 31 + 5).astype(np.int32)
    c['key'][:4] = (-2 ** 31, 2 ** 31 - 1, 0, -1)
    bad, ref = _check(dev, c, 'shuffled')
    print('FANIN shuffled | %d fan-ins listed | %d complaints' % (int((ref[0] >= 0).sum()), len(bad)))
    assert not bad, '\n'.join(bad)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_are_return_codes_with_every_output_untouched():
    dev = _dev()
    c = FR.decode_case(H=16, N=40, keys='asc', K=3)

    def refused(want_rc, K=None, H=None, gp='keep', mutate=None):
        cc = dict(c)
        if gp != 'keep':
            cc['graph_ptr'] = gp
        d = Decode(dev, cc, True, K=K, H=H)
        if mutate is not None:
            mutate(d)
        rc = d.rc()
        assert (rc, d.untouched()) == (want_rc, True), (rc, want_rc, K, H, gp)

    refused(MGV_EUNSUPPORTED, H=48)
    refused(MGV_EUNSUPPORTED, H=8)
    for K in (0, -1, 9):
        refused(MGV_EINVAL, K=K)
    refused(MGV_EINVAL, gp=[0, 10, 39])                       # does not end at N
    refused(MGV_EINVAL, gp=[0, 10, 41])
    refused(MGV_EINVAL, gp=[1, 10, 40])                       # does not start at 0
    for name in ('key', 'want'):
        refused(MGV_EINVAL, mutate=lambda d, name=name: setattr(d, name, None))
    d = Decode(dev, dict(c, graph_ptr=[0, 10, 40]), True)
    assert d.rc() == 0 and not d.untouched()
    from deepgate import _hip, ops
    s = c['s'].to(dev)
    with pytest.raises(_hip.HipLibraryError, match='EINVAL'):
        ops.fanin_decode(s, s, c['key'], c['want'], K=9)
    with pytest.raises(_hip.HipLibraryError, match='EINVAL'):
        ops.fanin_decode(s, s, c['key'], c['want'], graph_ptr=[0, 10, 39])
    with pytest.raises(_hip.HipLibraryError, match='one entry per node'):
        ops.fanin_decode(s, s, c['key'][:-1], c['want'])
    e = ops.fanin_decode(s[:0], s[:0], c['key'][:0], c['want'][:0], K=2)
    assert e[0].shape == (0, 2) and e[2].shape == (0,)


# ------------------------------------------------------------------------------------------------ the surface
def test_surface_matches_the_abi_and_takes_column_halves():
    dev = _dev()
    from deepgate import ops
    c = FR.decode_case(H=64, sizes=FR.SIZES, keys='levels', K=3)
    ref = Decode(dev, c, True).run().result()
    st = torch.cat([c['s'], c['t']], dim=1).to(dev)                          # the two halves of one array, as on the models
    for skip in (True, False):
        idx, score, n_cand = ops.fanin_decode(st[:, :64], st[:, 64:], c['key'], torch.from_numpy(c['want']), graph_ptr=c['graph_ptr'], K=3, skip=skip)
        assert idx.dtype == I32 and n_cand.dtype == I32 and FR.same_decode((idx.cpu().numpy(), score.cpu().numpy(), n_cand.cpu().numpy()), ref)
    # K defaults to want.max() clamped to 8
    idx, _, _ = ops.fanin_decode(st[:, :64], st[:, 64:], c['key'], c['want'], graph_ptr=c['graph_ptr'])
    assert int(c['want'].max()) == 8 and idx.shape == (c['N'], 8)                        # (the case's row that wants K + 5)
    assert np.array_equal(idx.cpu().numpy(), Decode(dev, c, True, K=8).run().result()[0])
    ei = ops.fanin_edges(torch.from_numpy(ref[0]).to(dev))
    keep = ref[0] >= 0
    assert ei.dtype == I64 and ei.shape == (2, int(keep.sum())) and np.array_equal(ei[0].cpu().numpy(), ref[0][keep])
    assert np.array_equal(ei[1].cpu().numpy(), np.repeat(np.arange(c['N']), 3).reshape(-1, 3)[keep])
    from deepgate.digae_layer import DirectedInnerProductDecoder
    d2 = DirectedInnerProductDecoder().decode_fanins(st[:, :64], st[:, 64:], c['key'], c['want'], graph_ptr=c['graph_ptr'], K=3)
    assert FR.same_decode(tuple(x.cpu().numpy() for x in d2), ref)


# ------------------------------------------------------------------------------------------------ recovery
def _recovery(dev, idx, edge_index, gp, with_hits=True):
    """mgv_fanin_recovery through the raw ABI on the true lists ops.true_fanin_lists builds -> (n_hit Out or None, rec Out)."""
    from deepgate import ops
    N, K = idx.shape
    tru_ptr, tru_src = ops.true_fanin_lists(torch.as_tensor(edge_index).to(dev), N)
    idxd = torch.as_tensor(idx).to(dev).contiguous()
    gpd = None if gp is None else torch.tensor(gp, dtype=I32, device=dev)
    G = 0 if gp is None else len(gp) - 1
    n_hit, rec = (Out(N, 1, dev, dtype=I32) if with_hits else None), Out(max(G, 1), 5, dev, dtype=I64)
    _call('mgv_fanin_recovery', N, K, _ptr(idxd), _ptr(tru_ptr), _ptr(tru_src), _ptr(gpd), G, None if n_hit is None else _ptr(n_hit.v), _ptr(rec.v))
    return n_hit, rec


def test_recovery_equals_the_set_restatement_on_designed_lists():
    """Empty true lists, a decoded -1, ids out of range, repeated true edges, graphs without gates, an empty graph, graphs across
    workgroup borders (tests/fanin_decode_ref.py recovery_case); with and without graph_ptr and n_hit; two calls, the same bytes."""
    dev = _dev()
    from deepgate import ops
    c = FR.recovery_case()
    for gp in (c['graph_ptr'], None):
        ref_hit, ref_rec = FR.recovery_ref(c['idx'], c['edge_index'], gp)
        n_hit, rec = _recovery(dev, c['idx'], c['edge_index'], gp)
        assert n_hit.intact() and rec.intact()
        assert np.array_equal(n_hit.v.flatten().cpu().numpy(), ref_hit) and np.array_equal(rec.v.cpu().numpy(), ref_rec), gp
        _, rec2 = _recovery(dev, c['idx'], c['edge_index'], gp, with_hits=False)
        assert torch.equal(rec2.parent, rec.parent)
        print('FANIN recovery graphs=%s | gates %d exact %d hits %d true %d decoded %d'
              % ((gp is not None,) + tuple(int(x) for x in ref_rec.sum(0))))
    r = ops.fanin_recovery(torch.from_numpy(c['idx']).to(dev), torch.from_numpy(c['edge_index']).to(dev), graph_ptr=c['graph_ptr'])
    ref_hit, ref_rec = FR.recovery_ref(c['idx'], c['edge_index'], c['graph_ptr'])
    assert r.counts.dtype == I64 and np.array_equal(r.counts.cpu().numpy(), ref_rec) and np.array_equal(r.n_hit.cpu().numpy(), ref_hit)
    rate = r.recovery.cpu().numpy()
    assert rate.dtype == np.float64 and np.array_equal(rate == -1, ref_rec[:, 0] == 0)            # -1 where a graph has no gate
    has = ref_rec[:, 0] > 0
    assert np.array_equal(rate[has], ref_rec[has, 1] / ref_rec[has, 0])
    assert np.array_equal(r.recall.cpu().numpy()[has], ref_rec[has, 2] / ref_rec[has, 3])
    # refusals: return codes, rec untouched
    idxd = torch.from_numpy(c['idx']).to(dev)
    tp, ts = ops.true_fanin_lists(torch.from_numpy(c['edge_index']).to(dev), c['N'])
    rec = Out(6, 5, dev, dtype=I64)
    bad_gp = torch.tensor([0, 10, c['N'] - 1], dtype=I32, device=dev)
    assert _rc('mgv_fanin_recovery', c['N'], 3, _ptr(idxd), _ptr(tp), _ptr(ts), _ptr(bad_gp), 2, None, _ptr(rec.v)) == MGV_EINVAL
    late, neg = tp.clone(), tp.clone()
    late[0], neg[-1] = 1, -1                                   # a table that does not start at 0; an end below 0
    for bad_tp in (late, neg):
        assert _rc('mgv_fanin_recovery', c['N'], 3, _ptr(idxd), _ptr(bad_tp), _ptr(ts), None, 0, None, _ptr(rec.v)) == MGV_EINVAL
    assert _rc('mgv_fanin_recovery', c['N'], 3, _ptr(idxd), _ptr(tp), None, None, 0, None, _ptr(rec.v)) == MGV_EINVAL
    assert _rc('mgv_fanin_recovery', c['N'], 0, _ptr(idxd), _ptr(tp), _ptr(ts), None, 0, None, _ptr(rec.v)) == MGV_EINVAL
    assert rec.untouched()


@pytest.mark.parametrize('H', HS)
def test_orthonormal_design_is_recovered_exactly(H):
    """True fan-ins score 1, everything else 0 (tests/fanin_decode_ref.py ortho_case; the restatement recovers it exactly on the CPU,
    tests/test_fanin_decode_spec.py): the device decodes every gate of every graph exactly."""
    dev = _dev()
    from deepgate import ops
    c = FR.ortho_case(H)
    bad, ref = _check(dev, c, 'H=%d ortho' % H)
    assert not bad, '\n'.join(bad)
    idx, _, n_cand = ops.fanin_decode(c['s'].to(dev), c['t'].to(dev), c['key'], c['want'], graph_ptr=c['graph_ptr'], K=3)
    r = ops.fanin_recovery(idx, torch.from_numpy(c['edge_index']).to(dev), graph_ptr=c['graph_ptr'])
    cnt = r.counts.cpu().numpy()
    print('FANIN ortho H=%d | per graph gates %s exact %s' % (H, cnt[:, 0].tolist(), cnt[:, 1].tolist()))
    assert (cnt[:, 0] > 0).all() and np.array_equal(cnt[:, 1], cnt[:, 0]) and bool((r.recovery == 1.0).all())
    assert np.array_equal(r.n_hit.cpu().numpy(), c['want']) and not bool((n_cand.cpu() < torch.from_numpy(c['want'])).any())


# ------------------------------------------------------------------------------------------------ legality, and the models
def _batch(ctype, dev, n=4):
    import deepgate
    from deepgate import synthetic as syn
    graphs = [syn.make_graph(ctype, 96, 10, 4400 + i, n_inputs=16) for i in range(n)]
    return deepgate.CircuitBatch.from_arrays(syn.collate(graphs), device=dev)


def _model(ctype, dev, H=64, variational=False):
    import deepgate
    torch.manual_seed(3)
    enc = deepgate.digae_layer.DirectMultiGCNEncoder(dim_feature=6, dim_hidden=H, s_rounds=1, t_rounds=1, layernorm=True)
    return getattr(deepgate, 'dg_ae_model_' + ctype).Model(struct_encoder=enc, dim_hidden=H, variational=variational).to(dev).eval()


def _legal(dec, batch, want):
    """Every decoded edge inside its graph and from a lower level to a higher one; every in-degree min(want, candidates)."""
    ei = dec.edge_index.cpu()
    N = batch.num_nodes
    gp = batch.graph_ptr
    g = torch.bucketize(torch.arange(N), gp[1:], right=True)
    lv = batch.forward_level.cpu()
    assert bool((g[ei[0]] == g[ei[1]]).all()) and bool((lv[ei[0]] < lv[ei[1]]).all())
    n_cand = torch.stack([((g == g[v]) & (lv < lv[v])).sum() if want[v] > 0 else torch.tensor(0) for v in range(N)])
    deg = torch.bincount(ei[1], minlength=N)
    assert torch.equal(deg, torch.minimum(want.clamp(min=0).long(), n_cand))
    assert torch.equal(dec.short.cpu(), n_cand < want) and dec.fanin.shape[0] == N
    assert torch.equal((dec.fanin >= 0).sum(1).cpu(), deg) and ei.shape[1] == int(deg.sum())
    same = ei[1][1:] == ei[1][:-1]
    assert bool((ei[1][1:] >= ei[1][:-1]).all())                              # by target ...
    sc = dec.score.cpu()[dec.fanin.cpu() >= 0]
    assert bool((sc[1:] <= sc[:-1])[same].all())                               # ... then by rank


@pytest.mark.parametrize('ctype,variational', [('aig', False), ('xmg', False), ('aig', True)])
def test_decode_circuit_is_legal_and_levelises(ctype, variational):
    """4 synthetic graphs of 96 nodes, random hs: the decoded circuit has the library's arities, stays inside each graph, runs from
    lower to higher levels, and a GraphPlan built from it levelises on the device; circuit_recovery counts it against the true edges."""
    dev = _dev()
    import deepgate
    from deepgate.graph_plan import GraphPlan
    batch = _batch(ctype, dev)
    model = _model(ctype, dev, variational=variational)
    N = batch.num_nodes
    torch.manual_seed(11)
    hs = torch.randn(N, 64, device=dev)
    dec = model.decode_circuit(hs, batch)
    want = model.gate_arity(batch.gate.flatten()).cpu()
    assert torch.equal(want.long(), torch.bincount(batch.edge_index[1].cpu(), minlength=N))      # the library arity is the true degree
    _legal(dec, batch, want)
    assert dec.fanin.shape[1] == (3 if ctype == 'xmg' else 2) and dec.edge_index.dtype == I64
    lv = GraphPlan(dec.edge_index, N).asap_levels().cpu()
    ei = dec.edge_index.cpu()
    assert bool((lv[ei[0]] < lv[ei[1]]).all()) and int(lv.max()) >= 1                              # acyclic: it levelises
    # the scores are the decoder's on the model's own halves (the posterior means of a variational model)
    s, t = model._decoder_halves(hs)
    at = deepgate.ops.pair_scores_at(s, t, dec.edge_index, sigmoid=False)
    assert torch.equal(_bits(at), _bits(dec.score[dec.fanin >= 0]))
    # want='degree' is the same on a circuit that obeys its library; a tensor and K are taken as given
    d2 = model.decode_circuit(hs, batch, want='degree')
    assert torch.equal(d2.fanin, dec.fanin) and torch.equal(d2.edge_index, dec.edge_index)
    d3 = model.decode_circuit(hs, batch, want=torch.ones(N, dtype=torch.int64), K=1)
    assert d3.fanin.shape == (N, 1) and torch.equal(d3.fanin[:, 0][want > 0].cpu(), dec.fanin[:, 0][want > 0].cpu())
    with pytest.raises(ValueError):
        model.decode_circuit(hs, batch, want='arity')
    rec, dec2 = model.circuit_recovery(hs, batch)
    assert torch.equal(dec2.fanin, dec.fanin)
    cnt = rec.counts.cpu().numpy()
    ref_hit, ref_rec = FR.recovery_ref(dec.fanin.cpu().numpy(), batch.edge_index.cpu().numpy(), batch.graph_ptr.tolist())
    assert np.array_equal(cnt, ref_rec) and np.array_equal(rec.n_hit.cpu().numpy(), ref_hit)
    assert (cnt[:, 0] == 80).all() and np.array_equal(cnt[:, 3], cnt[:, 4])                        # 80 gates per graph, all completed
    print('FANIN model %s variational=%s | per graph exact %s of %s gates, hits %s of %s'
          % (ctype, variational, cnt[:, 1].tolist(), cnt[:, 0].tolist(), cnt[:, 2].tolist(), cnt[:, 3].tolist()))
    # without forward_level on the batch the plan's ASAP levels are the key: the same circuit
    bare = _batch(ctype, dev)
    del bare.forward_level
    d4 = model.decode_circuit(hs, bare)
    assert torch.equal(d4.fanin, dec.fanin)


def test_directed_gae_carries_the_same_two():
    dev = _dev()
    import deepgate
    batch = _batch('aig', dev)
    model = _model('aig', dev)
    hs = torch.randn(batch.num_nodes, 64, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    s, t = model._decoder_halves(hs)
    gae = deepgate.digae_model.DirectedGAE(model.struct_encoder)
    want = model.gate_arity(batch.gate.flatten())
    dec = gae.decode_circuit(s, t, batch.forward_level, want, graph_ptr=batch.graph_ptr)
    ref = model.decode_circuit(hs, batch)
    assert all(torch.equal(a, b) for a, b in zip(dec, ref))
    rec, _ = gae.circuit_recovery(s, t, batch.edge_index, batch.forward_level, graph_ptr=batch.graph_ptr)        # want = the true degree
    assert torch.equal(rec.counts, model.circuit_recovery(hs, batch)[0].counts)


def test_feature_extract_decode_circuit(tmp_path, capsys):
    """examples/feature_extract.py --decode_circuit OUT.npz: per graph edge_index, fanin, score, short and the recovery record."""
    _dev()
    import importlib
    sys.path.insert(0, os.path.join(PKG_PARENT, 'examples'))
    fe = importlib.import_module('feature_extract')
    out, dec = tmp_path / 'emb.npz', tmp_path / 'dec.npz'
    fe.main(['--type', 'aig', '--synthetic', '3', '--rounds', '1', '--batch_size', '2', '--decode_circuit', str(dec), '--out', str(out)])
    z = np.load(dec)
    assert sorted(z.files) == sorted('graph%d/%s' % (i, k) for i in range(3) for k in ('edge_index', 'fanin', 'score', 'short', 'recovery'))
    assert sorted(np.load(out).files) == sorted('graph%d/%s' % (i, k) for i in range(3) for k in ('hs', 'hf'))
    for i in range(3):
        ei, fanin, short, rec = z['graph%d/edge_index' % i], z['graph%d/fanin' % i], z['graph%d/short' % i], z['graph%d/recovery' % i]
        n = fanin.shape[0]
        assert n == 1024 and fanin.shape == (n, 2) and fanin.dtype == np.int32 and short.dtype == np.bool_ and not short.any()
        assert ei.shape == (2, int((fanin >= 0).sum())) and ei.min() >= 0 and ei.max() < n and (ei[0] != ei[1]).all()   # local ids
        assert np.array_equal(ei[0], fanin[fanin >= 0]) and rec.shape == (5,) and rec[0] == 960 and 0 <= rec[1] <= rec[0]
        assert rec[3] == rec[4] == ei.shape[1]
    text = capsys.readouterr().out
    assert 'exact gate recovery over the 3 graphs with edges' in text


LINE_TODAY = r'val\| Epoch: \d+/\d+ \|Recon: \d+\.\d{4} \|ACC: \d+\.\d{2} \|Prob: \d+\.\d{4} \|Func: \d+\.\d{4}\|Net: \d+\.\d{2}s'


def test_trainer_val_line_with_val_recovery(tmp_path):
    """One epoch with --val_recovery on a synthetic set: the val line, and only it, carries ` |Recov: x.xxxx` at its end."""
    dev = _dev()
    import re
    import types

    import deepgate
    from deepgate import synthetic as syn
    from deepgate.trainer import GraphLoader
    if PKG_PARENT not in sys.path:
        sys.path.insert(0, PKG_PARENT)
    from config import get_parse_args
    assert get_parse_args(['--type', 'aig']).val_recovery is False and get_parse_args(['--type', 'aig', '--val_recovery']).val_recovery is True
    model = _model('aig', dev).train()
    graphs = [syn.make_graph('aig', 512, 10, 7700 + i, n_inputs=32) for i in range(4)]
    tr = deepgate.Trainer(types.SimpleNamespace(model='DG_AE', val_recovery=True), model, training_id='v', save_dir=str(tmp_path), lr=1e-4,
                          rc_prob_func_weight=[1.0, 4.0, 4.0], device='cuda:0', batch_size=2, distributed=False)
    tr.train(1, graphs, GraphLoader(graphs, 2, shuffle=False))
    lines = open(tr.log_path).read().splitlines()
    val, train = [ln for ln in lines if ln.startswith('val|')], [ln for ln in lines if ln.startswith('train|')]
    assert len(val) == 1 and len(train) == 1
    assert re.fullmatch(LINE_TODAY.replace('val', 'train', 1), train[0]), train[0]
    m = re.fullmatch(LINE_TODAY + r' \|Recov: (\d\.\d{4})', val[0])
    assert m, val[0]
    assert 0.0 <= float(m.group(1)) <= 1.0
