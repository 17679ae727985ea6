"""The connected-components entries — mgv_cc_init, mgv_cc_union_pairs, mgv_cc_labels, mgv_cc_class_count / mgv_cc_class_fill
(csrc/components.hip) and mgv_sim_union (csrc/pair_scores.hip) — through the C ABI and through the surface (ops.components /
class_table / sim_classes, Model.equivalence_classes, examples/feature_extract.py --classes), against tests/components_ref.py (pinned on
the CPU by tests/test_components_spec.py, which also asserts the properties of the builders used here and shows the planted defects of a
restated hook to be caught by the checkers used here).

Everything is integer work and compared EXACTLY: labels (the smallest id of a node's component), sizes, class_ptr, members; the
union-find's status record must be zeros.  mgv_sim_union is held to the components of the list mgv_sim_select_fill returns for the same
call; the cluster also to the float64 relation, whose band is empty (test_components_spec).

Conventions of tests/test_hip_embed_sim.py: raw ABI via its helpers, 64 guard entries behind every output, outputs filled with -77
before the call, parent filled with garbage before mgv_cc_init.  Every check prints one line `CC <what> | figures`."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_ref as CR  # noqa: E402
import embed_sim_ref as ER  # noqa: E402
import test_hip_embed_sim as TE  # noqa: E402  (SimRun and the device's own unit rows of the similarity cases)
import test_hip_pair_scores as TP  # noqa: E402

pytestmark = pytest.mark.gpu

F32, I32, I64 = torch.float32, torch.int32, torch.int64
HS = (16, 32, 64, 128)
MGV_EINVAL, MGV_EUNSUPPORTED = -1, -2
GARBAGE = 123456789
Out, _dev, _ptr, _rc, _call = TP.Out, TP._dev, TP._ptr, TP._rc, TP._call


class Forest:
    """parent [N] and status [4] with guards; parent holds garbage until mgv_cc_init."""

    def __init__(self, dev, N, init=True):
        self.N, self.dev = N, dev
        self.parent, self.status = Out(N, 1, dev, dtype=I32), Out(4, 1, dev, dtype=I32)
        self.parent.v.fill_(GARBAGE)
        if init:
            self.init()

    def init(self):
        _call('mgv_cc_init', self.N, _ptr(self.parent.v), _ptr(self.status.v))

    def union(self, pairs):
        p = pairs.to(self.dev)
        a, b = p[0].contiguous(), p[1].contiguous()
        _call('mgv_cc_union_pairs', self.N, a.numel(), _ptr(a), _ptr(b), _ptr(self.parent.v), _ptr(self.status.v))

    def labels(self):
        """(label, size) on the host, after checking the guards of all four arrays."""
        label, size = Out(self.N, 1, self.dev, dtype=I32), Out(self.N, 1, self.dev, dtype=I32)
        _call('mgv_cc_labels', self.N, _ptr(self.parent.v), _ptr(label.v), _ptr(size.v))
        self.intact = label.intact() and size.intact() and self.parent.intact() and self.status.intact()
        self.flat = torch.equal(self.parent.v, label.v)
        return label.v.flatten().cpu(), size.v.flatten().cpu()

    def code(self):
        return self.status.v.flatten().tolist()


@functools.lru_cache(maxsize=None)
def _list_refs():
    cases = CR.list_cases()
    return cases, {k: CR.uf_labels(c['pairs'], c['N']) for k, c in cases.items()}


def test_union_pairs_and_labels_on_the_designed_lists():
    dev = _dev()
    cases, refs = _list_refs()
    bad = []
    for name, c in cases.items():
        f = Forest(dev, c['N'])
        f.union(c['pairs'])
        label, size = f.labels()
        bad += ['%s: %s' % (name, b) for b in CR.check_components(label, size, refs[name])]
        if f.code() != [0, 0, 0, 0]:
            bad.append('%s: status %s' % (name, f.code()))
        if not (f.intact and f.flat):
            bad.append('%s: guard entries changed, or parent is not flattened to the labels' % name)
        print('CC list %-32s | N %5d | P %5d | %d components | status %s' % (name, c['N'], c['pairs'].shape[1],
                                                                             int((label == torch.arange(c['N'])).sum()), f.code()))
    assert not bad, bad[:10]


def test_forest_past_the_grid_cap_in_three_orders_and_twice():
    dev = _dev()
    N = CR.GRID_CAP_THREADS + 1
    c = CR.forest(N, 2 * N, 7)
    want = CR.propagate_labels(c['pairs'], N)
    g = torch.Generator().manual_seed(5)
    orders = {'as listed': c['pairs'], 'reversed': c['pairs'].flip(1), 'shuffled': c['pairs'][:, torch.randperm(2 * N, generator=g)],
              'as listed, again': c['pairs']}
    bad, got = [], {}
    for name, p in orders.items():
        f = Forest(dev, N)
        f.union(p)
        label, size = f.labels()
        got[name] = label
        bad += ['%s: %s' % (name, b) for b in CR.check_components(label, size, want)]
        if f.code() != [0, 0, 0, 0] or not f.intact:
            bad.append('%s: status %s, guards intact %s' % (name, f.code(), f.intact))
    first = got['as listed']
    assert all(torch.equal(first, v) for v in got.values())
    # the class table of a labelling with more than one scan block
    lab = first.to(device=dev, dtype=I32)
    for ms in (2, 5):
        bad += ['table min_size %d: %s' % (ms, b) for b in _table_raw(dev, lab, ms, first)]
    print('CC forest N=%d P=%d | %d components, largest %d | 4 runs, one labelling | %d findings'
          % (N, 2 * N, int((first == torch.arange(N)).sum()), int(CR.sizes_ref(first).max()), len(bad)))
    assert not bad, bad[:10]


def test_error_records_instead_of_faults():
    """An id outside [0, N) is skipped and recorded (code 3); a parent array that never went through mgv_cc_init is recognised at the
    first find (code 1): nothing outside the arrays is touched either way."""
    dev = _dev()
    from deepgate import _hip, ops
    N = 100
    pairs = torch.tensor([[3, 7, 100, 9, -1], [4, 8, 5, 2 ** 40, 6]], dtype=I64)
    f = Forest(dev, N)
    f.union(pairs)
    label, _ = f.labels()
    st = f.code()
    assert st[0] == 3 and f.intact
    assert CR.check_components(label, None, CR.uf_labels(pairs[:, :2], N)) == []
    with pytest.raises(_hip.HipLibraryError, match='outside'):
        ops.components(pairs.to(dev), N)
    g = Forest(dev, N, init=False)
    g.status.v.zero_()
    g.union(pairs[:, :2])
    assert g.code()[0] == 1 and g.code()[2] == GARBAGE and g.parent.intact() and bool((g.parent.v == GARBAGE).all())
    print('CC errors | id out of range: status %s | no init: status %s' % (st, g.code()))


# ------------------------------------------------------------------------------------------------ classes from the tile walk
@pytest.mark.parametrize('H', HS)
def test_sim_union_equals_the_components_of_the_selected_list(H):
    dev = _dev()
    bad, n_comp = [], []
    for kind in ER.CASES:
        c, _ = TE._case(H, 1, kind)
        gp, N, info = c['graph_ptr'], c['N'], c['info']
        y, _ = TE._device_rows(H, 1, kind)
        f = Forest(dev, N, init=False)                      # one forest through all thresholds: re-initialised before each
        first = torch.arange(N) if gp is None else ER.PR.row_range(gp, N)[0]
        for thr in ER.THRESHOLDS:
            tag = '%s H=%d thr=%g' % (kind, H, thr)
            run = TE.SimRun(dev, y, gp, thr, with_score=False)
            row_ptr, col, _ = run.lists()
            rows = torch.repeat_interleave(torch.arange(N), row_ptr[1:] - row_ptr[:-1])
            want = CR.uf_labels(torch.stack([rows, col.to(I64)]), N)
            f.init()
            _call('mgv_sim_union', *run.args, _ptr(f.parent.v), _ptr(f.status.v))
            label, size = f.labels()
            bad += ['%s: %s' % (tag, b) for b in CR.check_components(label, size, want)]
            if f.code() != [0, 0, 0, 0] or not f.intact:
                bad.append('%s: status %s, guards intact %s' % (tag, f.code(), f.intact))
            n_comp.append(int((label == torch.arange(N)).sum()))
            if thr == -2.0:
                if kind == 'nan':
                    ok = int(label[info['nan']]) == info['nan'] and int((label == 0).sum()) == N - 1
                else:
                    ok = torch.equal(label.to(I64), first)
                if not ok:
                    bad.append('%s: not one class per non-empty graph, labelled with its first node' % tag)
            if thr == 1.5 and not torch.equal(label.to(I64), torch.arange(N)):
                bad.append('%s: something is united above 1.5' % tag)
            if kind != 'nan' and info['border'] is not None and int(label[info['border'][0]]) == int(label[info['border'][1]]):
                bad.append('%s: the copy across the graph border is united' % tag)
            if thr == 0.999:
                alone = [info['nan']] if kind == 'nan' else info['zeros']
                if any(int(size[i]) != 1 or int(label[i]) != i for i in alone):
                    bad.append('%s: a NaN row or a zero row is no singleton' % tag)
                if kind == 'sim':
                    t0, t1, t2 = info['trio']
                    if not (int(label[t1]) == t0 and int(label[t2]) == t0 and int(label[info['near']]) == t0 and int(size[t0]) == 4):
                        bad.append('%s: the trio and its near-duplicate are not one class of 4' % tag)
    print('CC walk H=%d | %d configurations, %d .. %d components | %d findings' % (H, len(n_comp), min(n_comp), max(n_comp), len(bad)))
    assert not bad, bad[:10]


# ------------------------------------------------------------------------------------------------ the cluster
@functools.lru_cache(maxsize=None)
def _cluster(H):
    c = CR.cluster_case(H, 1)
    pairs, _, _ = CR.truth_pairs(c['x'], c['graph_ptr'], CR.SIM_THR)
    return c, pairs, CR.uf_labels(pairs, c['N'])


@pytest.mark.parametrize('H', (64, 16))
def test_cluster_one_class_of_300_on_both_routes(H):
    dev = _dev()
    from deepgate import _hip, ops
    c, pairs, want = _cluster(H)
    xd, gp, N = c['x'].to(dev), c['graph_ptr'], c['N']
    label, class_ptr, members = ops.sim_classes(xd, graph_ptr=gp, threshold=CR.SIM_THR, route='walk')
    assert label.dtype == I32 and class_ptr.dtype == I64 and members.dtype == I32 and label.is_cuda
    bad = CR.check_components(label, None, want) + CR.check_table(class_ptr, members, want, 2)
    lab = label.cpu()
    root = c['members'][0]
    assert torch.nonzero(lab == root).flatten().tolist() == c['members']
    assert int(lab[c['copy']]) == c['copy']                                     # the copy in the next graph stays outside
    assert all(int(lab[b]) == a for a, b in c['doubles'])
    sizes = (class_ptr[1:] - class_ptr[:-1]).tolist()
    assert sorted(sizes) == [2, 2, 2, 300] and members[class_ptr[:-1]].tolist() == sorted([root] + [a for a, _ in c['doubles']])
    # the pair list of this circuit is refused at a cap the classes never meet
    with pytest.raises(_hip.HipLibraryError, match='max_pairs'):
        ops.sim_pairs(xd, graph_ptr=gp, threshold=CR.SIM_THR, max_pairs=10_000)
    with pytest.raises(_hip.HipLibraryError, match='max_pairs'):
        ops.sim_classes(xd, graph_ptr=gp, threshold=CR.SIM_THR, route='pairs', max_pairs=10_000)
    pi = ops.sim_pairs(xd, graph_ptr=gp, threshold=CR.SIM_THR)[0]
    assert pi.shape[1] == pairs.shape[1] >= 44850
    via = ops.sim_classes(xd, graph_ptr=gp, threshold=CR.SIM_THR, route='pairs')
    for a, b, what in zip((label, class_ptr, members), via, ('label', 'class_ptr', 'members')):
        if not torch.equal(a, b):
            bad.append('the two routes differ in %s' % what)
    if not torch.equal(ops.components(pi, N), label):
        bad.append('ops.components of the pair list differs from the walk')
    # every min_size through the surface and through the raw entries
    for ms in (1, 2, 3, 301):
        cp, mem = ops.class_table(label, min_size=ms)
        bad += ['class_table min_size %d: %s' % (ms, b) for b in CR.check_table(cp, mem, want, ms)]
        bad += ['raw table min_size %d: %s' % (ms, b) for b in _table_raw(dev, label, ms, want)]
        if ms == 301 and not (cp.tolist() == [0] and mem.numel() == 0):
            bad.append('min_size 301 does not give the empty table')
    print('CC cluster H=%d | %d pairs, classes of %s | walk = pairs route = float64 relation | %d findings' % (H, pi.shape[1], sizes, len(bad)))
    assert not bad, bad[:10]


def _table_raw(dev, label, min_size, want):
    """mgv_cc_class_count / mgv_cc_class_fill through the raw ABI with guards -> findings."""
    from deepgate import _hip
    N = label.numel()
    ws_ints = _hip.call_value('mgv_cc_class_ws_ints', N)
    ws = torch.full((ws_ints + 64,), -77, dtype=I32, device=dev)
    counts = Out(6, 1, dev, dtype=I32)
    _call('mgv_cc_class_count', N, _ptr(label), min_size, None, _ptr(ws), ws_ints, _ptr(counts.v))
    C, M = counts.v.flatten().tolist()[:2]
    if counts.v.flatten().tolist()[2:] != [0, 0, 0, 0] or not counts.intact() or not bool((ws[ws_ints:] == -77).all()):
        return ['counts %s, or guard entries changed' % counts.v.flatten().tolist()]
    class_ptr, members = Out(C + 1, 1, dev, dtype=I64), Out(M, 1, dev, dtype=I32)
    temp_ints = _hip.call_value('mgv_sort_pairs_temp_ints', 4, max(M, 1))
    temp = torch.empty(temp_ints, dtype=I32, device=dev)
    _call('mgv_cc_class_fill', N, _ptr(label), C, M, _ptr(ws), ws_ints, _ptr(temp), temp_ints, _ptr(class_ptr.v), _ptr(members.v))
    bad = CR.check_table(class_ptr.v, members.v, want, min_size)
    if not (class_ptr.intact() and members.intact() and bool((ws[ws_ints:] == -77).all())):
        bad.append('guard entries changed')
    return bad


# ------------------------------------------------------------------------------------------------ surface
def test_the_model_method_the_decoder_lists_and_small_inputs():
    dev = _dev()
    import deepgate
    from deepgate import ops, synthetic as syn
    H = 64
    torch.manual_seed(0)
    enc = deepgate.digae_layer.DirectMultiGCNEncoder(dim_feature=6, dim_hidden=H, s_rounds=1, t_rounds=1, layernorm=True)
    model = deepgate.dg_ae_model_aig.Model(struct_encoder=enc, dim_hidden=H).to(dev).eval()
    graphs = [syn.make_graph('aig', 300, 12, 50 + i, n_inputs=24) for i in range(3)]
    batch = deepgate.CircuitBatch.from_arrays(syn.collate(graphs), device=dev)
    with torch.no_grad():
        hs, hf = model(batch)
    N = hf.shape[0]
    found = []
    for thr in (0.999, 0.9):
        label, class_ptr, members = model.equivalence_classes(hf, graph_ptr=batch.graph_ptr, threshold=thr)
        pi = model.equivalence_candidates(hf, graph_ptr=batch.graph_ptr, threshold=thr)[0]
        assert torch.equal(label, ops.components(pi, N))
        want = CR.bfs_labels(pi.cpu(), N)
        assert CR.check_components(label, None, want) == [] and CR.check_table(class_ptr, members, want, 2) == []
        lab = label.cpu().to(I64)
        assert bool((lab // 300 == torch.arange(N) // 300).all())                # classes never cross graphs
        inputs = torch.nonzero(hf.abs().sum(1) == 0).flatten().cpu()
        assert inputs.numel() >= 3 * 24 and torch.equal(lab[inputs], inputs) and not bool(torch.isin(members.cpu().to(I64), inputs).any())
        found.append((pi.shape[1], class_ptr.numel() - 1, members.numel()))
    # components of a decoded link list (direction ignored)
    ei = model.reconstruct_edges(hs, graph_ptr=batch.graph_ptr, threshold=0.5)[0]
    lab = ops.components(ei, N)
    assert CR.check_components(lab, None, CR.bfs_labels(ei.cpu(), N)) == []
    # small inputs
    empty = torch.zeros((2, 0), dtype=I64, device=dev)
    assert ops.components(empty, 5).tolist() == [0, 1, 2, 3, 4] and ops.components(empty, 0).shape == (0,)
    cp, mem = ops.class_table(torch.zeros(0, dtype=I32, device=dev))
    assert cp.tolist() == [0] and mem.shape == (0,)
    label, cp, mem = ops.sim_classes(torch.zeros(0, 16, device=dev), graph_ptr=[0])
    assert label.shape == (0,) and cp.tolist() == [0] and mem.shape == (0,)
    label, cp, mem = ops.sim_classes(torch.ones(3, 16, device=dev), threshold=0.5, min_size=1)
    assert label.tolist() == [0, 0, 0] and cp.tolist() == [0, 3] and mem.tolist() == [0, 1, 2]
    print('CC model N=%d | (pairs, classes, members) at 0.999 and 0.9: %s | decoded list of %d links: %d components'
          % (N, found, ei.shape[1], int((lab.cpu() == torch.arange(N)).sum())))


def test_feature_extract_classes(tmp_path):
    """examples/feature_extract.py --classes THR: name/eq_label, name/eq_class_ptr and name/eq_members with ids local to the graph."""
    _dev()
    import importlib

    import numpy as np
    from conftest import PKG_PARENT
    sys.path.insert(0, os.path.join(PKG_PARENT, 'examples'))
    fe = importlib.import_module('feature_extract')
    out = tmp_path / 'emb.npz'
    fe.main(['--type', 'aig', '--synthetic', '2', '--rounds', '1', '--batch_size', '2', '--classes', '0.999', '--equivalences', '0.999',
             '--out', str(out)])
    emb = np.load(out)
    assert sorted(emb.files) == sorted('graph%d/%s' % (i, k) for i in range(2) for k in ('hs', 'hf', 'eq_label', 'eq_class_ptr', 'eq_members',
                                                                                       'eq_pairs', 'eq_cos'))
    for i in range(2):
        n = emb['graph%d/hf' % i].shape[0]
        label, cp, mem = emb['graph%d/eq_label' % i], emb['graph%d/eq_class_ptr' % i], emb['graph%d/eq_members' % i]
        assert label.shape == (n,) and label.dtype == np.int32 and mem.dtype == np.int32 and cp.dtype == np.int64
        want = CR.bfs_labels(torch.from_numpy(emb['graph%d/eq_pairs' % i].astype(np.int64)), n)          # local ids on both sides
        assert CR.check_components(torch.from_numpy(label), None, want) == []
        assert CR.check_table(torch.from_numpy(cp), torch.from_numpy(mem), want, 2) == []


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_are_return_codes_with_every_output_untouched():
    dev = _dev()
    n = 40
    y48, y = torch.randn(n, 48, device=dev), torch.randn(n, 16, device=dev)

    def union(H, N, x, ld, gp=None, parent=True, status=True):
        f = Forest(dev, n, init=False)
        f.parent.parent.fill_(-77)
        gpd = None if gp is None else torch.tensor(gp, dtype=I32, device=dev)
        rc = _rc('mgv_sim_union', H, N, _ptr(x), ld, _ptr(gpd), 0 if gp is None else len(gp) - 1, 0.5,
                 _ptr(f.parent.v) if parent else None, _ptr(f.status.v) if status else None)
        return rc, f.parent.untouched() and f.status.untouched()
    assert union(48, n, y48, 48) == (MGV_EUNSUPPORTED, True)
    assert union(0, n, y, 16) == (MGV_EUNSUPPORTED, True)
    assert union(16, -1, y, 16) == (MGV_EINVAL, True)
    assert union(16, 2 ** 31, y, 16) == (MGV_EINVAL, True)
    assert union(16, n, y, 12) == (MGV_EINVAL, True)                              # row stride below H
    assert union(16, n, y, 18) == (MGV_EINVAL, True)                              # row stride no multiple of 4
    assert union(16, n, y, 16, parent=False) == (MGV_EINVAL, True)
    assert union(16, n, y, 16, status=False) == (MGV_EINVAL, True)
    assert union(16, n, y, 16, gp=[0, 10, n - 1]) == (MGV_EINVAL, True)           # does not end at N
    assert union(16, 0, y, 16) == (0, True)                                       # nothing is launched
    # the list entries
    f = Forest(dev, n, init=False)
    f.parent.parent.fill_(-77)
    label, size = Out(n, 1, dev, dtype=I32), Out(n, 1, dev, dtype=I32)
    a = torch.zeros(4, dtype=I64, device=dev)
    P, S, L = _ptr(f.parent.v), _ptr(f.status.v), _ptr(label.v)
    assert _rc('mgv_cc_init', -1, P, S) == MGV_EINVAL and _rc('mgv_cc_init', n, None, S) == MGV_EINVAL
    assert _rc('mgv_cc_init', n, P, None) == MGV_EINVAL and _rc('mgv_cc_init', 2 ** 31, P, S) == MGV_EINVAL
    assert _rc('mgv_cc_union_pairs', -1, 4, _ptr(a), _ptr(a), P, S) == MGV_EINVAL
    assert _rc('mgv_cc_union_pairs', n, -1, _ptr(a), _ptr(a), P, S) == MGV_EINVAL
    assert _rc('mgv_cc_union_pairs', n, 4, None, _ptr(a), P, S) == MGV_EINVAL
    assert _rc('mgv_cc_union_pairs', n, 4, _ptr(a), _ptr(a), None, S) == MGV_EINVAL
    assert _rc('mgv_cc_union_pairs', n, 4, _ptr(a), _ptr(a), P, None) == MGV_EINVAL
    assert _rc('mgv_cc_labels', -1, P, L, _ptr(size.v)) == MGV_EINVAL and _rc('mgv_cc_labels', n, None, L, _ptr(size.v)) == MGV_EINVAL
    assert _rc('mgv_cc_labels', n, P, None, _ptr(size.v)) == MGV_EINVAL
    ws = torch.full((4096,), -77, dtype=I32, device=dev)
    counts = Out(6, 1, dev, dtype=I32)
    lab = torch.zeros(n, dtype=I32, device=dev)
    assert _rc('mgv_cc_class_count', n, _ptr(lab), 0, None, _ptr(ws), 4096, _ptr(counts.v)) == MGV_EINVAL        # min_size < 1
    assert _rc('mgv_cc_class_count', n, _ptr(lab), 2, None, _ptr(ws), 10, _ptr(counts.v)) == MGV_EINVAL          # workspace too short
    assert _rc('mgv_cc_class_count', n, None, 2, None, _ptr(ws), 4096, _ptr(counts.v)) == MGV_EINVAL
    assert _rc('mgv_cc_class_fill', n, _ptr(lab), 3, 2, _ptr(ws), 4096, None, 0, _ptr(a), _ptr(lab)) == MGV_EINVAL   # C > M
    assert f.parent.untouched() and f.status.untouched() and label.untouched() and size.untouched() and counts.untouched()
    assert bool((ws == -77).all())
