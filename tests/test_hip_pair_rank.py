"""The rank entry of csrc/pair_scores.hip — mgv_pair_rank_counts — through the C ABI and through the surface (ops.pair_rank_counts /
link_ranks / rank_metrics, DirectedInnerProductDecoder.rank, Model.link_ranking, DirectedGAE.link_ranking, examples/feature_extract.py
--link_ranking), against tests/pair_rank_ref.py (pinned on the CPU by tests/test_pair_rank_spec.py).

Every comparison is integer equality: the counts equal the plain-loop counts over the device's own dense scores (mgv_pair_scores_fwd on
the same operands: the bits the walk compares) under the reference's candidate masks, and they equal what the entries the project
already trusts say — mgv_pair_select_count at one threshold, counts_above of mgv_pair_hist at a table, the positions of mgv_pair_topk.

Conventions of tests/test_hip_pair_scores.py: operands are column slices of wider matrices whose foreign columns hold NaN; n_gt and
n_eq have 64 guard words behind them and hold -77 before the call.  Every check prints one line `RANK <what> | figures`."""
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_hist_ref as HR  # noqa: E402
import pair_rank_ref as RR  # noqa: E402
import pair_scores_ref as PR  # noqa: E402
import test_hip_pair_scores as TP  # noqa: E402  (the operand slices and the launcher helpers of the pair-score tests)

pytestmark = pytest.mark.gpu

F64, F32, I32, I64 = torch.float64, torch.float32, torch.int32, torch.int64
HS = (16, 32, 64, 128)
NS = (1, 63, 64, 65, 129, 200)
GUARD = TP.GUARD
FILL = -77
NAN = float('nan')
MGV_EINVAL, MGV_EUNSUPPORTED = -1, -2
_dev, _ptr, _rc, _call, _slice = TP._dev, TP._ptr, TP._rc, TP._call, TP._slice
LENGTHS = (0, 1, 32, 33, 65)                                # both sides of the pass boundary, and a third pass


class Counts:
    """n_gt and n_eq, int32 [T] each with GUARD words behind, -77 everywhere before the call."""

    def __init__(self, T, dev):
        self.T = T
        self.gt = torch.full((T + GUARD,), FILL, dtype=I32, device=dev)
        self.eq = torch.full((T + GUARD,), FILL, dtype=I32, device=dev)

    def intact(self):
        return bool((self.gt[self.T:] == FILL).all()) and bool((self.eq[self.T:] == FILL).all())

    def untouched(self):
        return bool((self.gt == FILL).all()) and bool((self.eq == FILL).all())

    def host(self):
        return self.gt[:self.T].cpu().numpy().astype(np.int64), self.eq[:self.T].cpu().numpy().astype(np.int64)


class Walk:
    """The operands of one case on the device (strided) and the entry on them."""

    def __init__(self, dev, s, t, gp):
        self.dev, self.gp = dev, gp
        self.N, self.H = s.shape
        self.sv, self.lds = _slice(s, dev)
        self.tv, self.ldt = _slice(t, dev)
        self.gpd = None if gp is None else torch.tensor(gp, dtype=I32, device=dev)
        self.G = 0 if gp is None else len(gp) - 1
        self.dense = TP._fwd(dev, s, t, False)[0].v.cpu().numpy() if self.N else np.zeros((0, 0), np.float32)

    def rank(self, tp, th, skip, out=None):
        tpd = torch.as_tensor(np.asarray(tp, dtype=np.int32), device=self.dev)
        thd = torch.as_tensor(np.asarray(th, dtype=np.float32), device=self.dev)
        c = Counts(thd.numel(), self.dev) if out is None else out
        _call('mgv_pair_rank_counts', self.H, self.N, _ptr(self.sv), self.lds, _ptr(self.tv), self.ldt, _ptr(self.gpd), self.G, int(skip),
              _ptr(tpd), _ptr(thd), _ptr(c.gt), _ptr(c.eq))
        return c


def _row_lists(dense, lengths, seed):
    """(thr_ptr, thr sorted per row): row u lists lengths[u] values drawn with repeats from its own scores bit for bit, their two
    float32 neighbours, -inf, +inf and NaN — `>` and `==` flip exactly at a score."""
    N = dense.shape[0]
    rng = np.random.RandomState(seed)
    tp = np.zeros(N + 1, dtype=np.int64)
    tp[1:] = np.cumsum(lengths)
    th = np.zeros(int(tp[-1]), dtype=np.float32)
    for u in range(N):
        row = dense[u][~np.isnan(dense[u])]
        if row.size == 0:
            row = np.zeros(1, np.float32)
        pool = np.concatenate([row, np.nextafter(row, np.float32(np.inf)), np.nextafter(row, np.float32(-np.inf)),
                               np.array([-np.inf, np.inf, NAN], np.float32)]).astype(np.float32)
        w = np.concatenate([np.full(3 * row.size, 1.0), np.full(3, 0.02 * 3 * row.size)])
        th[tp[u]:tp[u + 1]] = pool[rng.choice(pool.size, size=lengths[u], p=w / w.sum())]
    return tp.astype(np.int32), RR.sorted_lists(tp, th)[0]


def _check(tag, walk, tp, th, skip, twice=False):
    bad = []
    c = walk.rank(tp, th, skip)
    gt, eq = c.host()
    want_gt, want_eq = RR.rank_counts_ref(walk.dense, tp, th, walk.gp, skip)
    if not (np.array_equal(gt, want_gt) and np.array_equal(eq, want_eq)):
        d = np.nonzero((gt != want_gt) | (eq != want_eq))[0]
        j = int(d[0])
        bad.append('%s: %d of %d entries differ, first j=%d (thr %r): (%d, %d), expected (%d, %d)'
                   % (tag, d.size, gt.size, j, float(th[j]), gt[j], eq[j], want_gt[j], want_eq[j]))
    if not c.intact():
        bad.append('%s: the words behind an output changed' % tag)
    if twice:
        first = (c.gt.clone(), c.eq.clone())
        c2 = walk.rank(tp, th, skip)
        if not (torch.equal(c2.gt, first[0]) and torch.equal(c2.eq, first[1])):
            bad.append('%s: a second call gives other bytes' % tag)
    return bad, gt.size


def _tables(N):
    out = [None, [0, N]]
    if N == 129:
        out.append([0, 5, 70, 129])                         # graphs cut by a tile edge, a tile holding three graphs
    if N > 5:
        out.append([0, 5, 5, N])                            # an empty graph
    return out


# ------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize('H', HS)
def test_counts_equal_the_plain_loops_over_the_devices_own_scores(H):
    """N in NS, every table of _tables, skip_self off and on; list lengths 0, 1, 32, 33, 65 by row; at N = 129 also a NaN row in t
    (column 7 is nobody's candidate) and one in s (row 70 counts nothing)."""
    dev = _dev()
    bad, entries, runs = [], 0, 0
    for N in NS:
        s, t = RR.float_case(N, H, 1)
        cases = [(s, t, '')]
        if N == 129:
            s2, t2 = s.clone(), t.clone()
            t2[7], s2[70] = NAN, NAN
            cases.append((s2, t2, ' NaN rows'))
        for sx, tx, what in cases:
            for gp in _tables(N):
                walk = Walk(dev, sx, tx, gp)
                lengths = [LENGTHS[(u + N) % 5] for u in range(N)]
                tp, th = _row_lists(walk.dense, lengths, 11 * N + H)
                for skip in (False, True):
                    tag = 'H=%d N=%d%s graphs=%s skip_self=%s' % (H, N, what, gp, skip)
                    b, n = _check(tag, walk, tp, th, skip, twice=N >= 129)
                    bad += b
                    entries += n
                    runs += 1
    print('RANK exact H=%d | %d walks, %d listed thresholds | %d findings' % (H, runs, entries, len(bad)))
    assert not bad, bad[:10]


@pytest.mark.parametrize('H', (16, 128))
def test_a_hub_row_among_rows_that_list_nothing_and_no_list_at_all(H):
    dev = _dev()
    N = 200
    s, t = RR.float_case(N, H, 2)
    bad = []
    for gp in (None, [0, 5, 70, 200]):
        walk = Walk(dev, s, t, gp)
        lengths = [u % 2 for u in range(N)]
        lengths[66] = 300                                   # ten passes of the second tile; the first and the last tile do one
        tp, th = _row_lists(walk.dense, lengths, 5)
        b, n = _check('hub H=%d graphs=%s' % (H, gp), walk, tp, th, True, twice=True)
        bad += b
        lengths = [0] * N
        lengths[130] = 40                                   # two tiles whose rows list nothing walk nothing
        tp, th = _row_lists(walk.dense, lengths, 6)
        bad += _check('one row H=%d graphs=%s' % (H, gp), walk, tp, th, False)[0]
        c = walk.rank(np.zeros(N + 1, np.int32), np.zeros(0, np.float32), False)      # T = 0
        assert c.untouched()
    print('RANK hub H=%d | %d findings' % (H, len(bad)))
    assert not bad, bad[:10]


def test_a_thr_ptr_that_wanders_between_its_ends_stays_inside_the_lists():
    """Whatever thr_ptr holds between 0 and T, a row's range is clamped into [0, T): row 4 ends at -4 (empty), row 5 runs from 0 to 2^30
    (all of thr: 13 passes over a list that does not ascend, whose counts mean nothing) and row 6 starts there (empty).  The call
    returns, the words behind both outputs stay, and the rows of the other tiles list what they listed."""
    dev = _dev()
    N, H = 129, 32
    s, t = RR.float_case(N, H, 3)
    walk = Walk(dev, s, t, [0, 64, 129])
    tp, th = _row_lists(walk.dense, [3] * N, 7)
    tp = tp.copy()
    tp[5], tp[6] = -4, 2 ** 30
    c = walk.rank(tp, th, False)
    torch.cuda.synchronize()
    assert c.intact()
    assert not (c.gt[:c.T] == FILL).any() and not (c.eq[:c.T] == FILL).any()          # row 5 listed everything


# ------------------------------------------------------------------------------------------------ against the entries the project trusts
@pytest.mark.parametrize('H', HS)
def test_cross_checks_with_the_count_the_profile_and_the_topk_entries(H):
    dev = _dev()
    from deepgate import ops
    c = PR.topk_case(H, 1)
    gp, N = c['graph_ptr'], c['N']
    walk = Walk(dev, c['s'], c['t'], gp)
    sd, td = c['s'].to(dev), c['t'].to(dev)
    # one threshold x in every row: n_gt is n_sel of the count entry
    for x, skip in ((0.0, False), (0.75, True), (-3.5, False)):
        tp, th = np.arange(N + 1, dtype=np.int32), np.full(N, x, np.float32)
        gt, _ = walk.rank(tp, th, skip).host()
        n_sel = torch.full((N,), FILL, dtype=I32, device=dev)
        _call('mgv_pair_select_count', H, N, _ptr(walk.sv), walk.lds, _ptr(walk.tv), walk.ldt, _ptr(walk.gpd), walk.G, 0, x, int(skip),
              _ptr(n_sel))
        assert np.array_equal(gt, n_sel.cpu().numpy()), (H, x, skip)
    # the table `edges` in every row: per graph, the sums of n_gt are counts_above of the profile
    for name in ('A', 'D'):
        e = HR.edges_f32(name)
        B = e.numel()
        tp, th = (B * np.arange(N + 1)).astype(np.int32), np.tile(e.numpy(), N)
        gt, _ = walk.rank(tp, th, False).host()
        per_row = torch.from_numpy(gt.reshape(N, B))
        gid = HR.graph_ids(gp, N)[0]
        sums = torch.zeros((len(gp) - 1, B), dtype=I64).index_add_(0, gid, per_row)
        prof = ops.pair_profile(sd, td, e, graph_ptr=gp, sigmoid=False, skip_self=False)
        assert torch.equal(sums, ops.counts_above(prof).cpu()), (H, name)
    # a link the top-k list holds at position p has n_gt <= p < n_gt + n_eq
    ei = torch.unique(PR.edges_case(c, 3, 1), dim=1).to(dev)
    for skip in (False, True):
        thr = ops.pair_scores_at(sd, td, ei, sigmoid=False)
        lists = ops.link_rank_lists(ei, thr, N, graph_ptr=gp, by='src', skip_self=skip)
        n_gt, n_eq = ops.pair_rank_counts(sd, td, lists.thr_ptr, lists.thr, graph_ptr=gp, skip_self=skip)
        idx, _, _ = ops.pair_topk(sd, td, 32, graph_ptr=gp, sigmoid=False, skip_self=skip)
        col = ei[1][lists.perm]
        hit = (idx[lists.row].long() == col[:, None])
        found = hit.any(1) & lists.valid
        p = hit.float().argmax(1)
        assert int(found.sum()) > 100
        assert bool((n_eq[lists.valid] >= 1).all())                                    # a valid link finds itself
        assert bool(((n_gt.long() <= p) & (p < n_gt.long() + n_eq.long()))[found].all()), (H, skip)
    print('RANK cross H=%d | count entry at 3 thresholds, profile tables A and D, %d links in the top-32 lists | ok' % (H, int(found.sum())))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_are_return_codes_and_the_outputs_stay_untouched():
    dev = _dev()
    n = 40
    y48, y = torch.randn(n, 48, device=dev), torch.randn(n, 16, device=dev)
    T = 2 * n
    good_tp = torch.arange(0, T + 1, 2, dtype=I32, device=dev)
    thr = torch.zeros(T, device=dev)

    def run(H, N, x, ld, gp, tp=good_tp, th=thr, base=None, gt=True, eq=True):
        gpd = None if gp is None else torch.tensor(gp, dtype=I32, device=dev)
        G = 0 if gp is None else len(gp) - 1
        c = Counts(T, dev)
        xp = _ptr(x) if base is None else base
        rc = _rc('mgv_pair_rank_counts', H, N, xp, ld, xp, ld, _ptr(gpd), G, 0, _ptr(tp), _ptr(th), _ptr(c.gt) if gt else None,
                 _ptr(c.eq) if eq else None)
        torch.cuda.synchronize()
        return rc, c.untouched()
    INV, UNS = (MGV_EINVAL, True), (MGV_EUNSUPPORTED, True)
    assert run(48, n, y48, 48, None) == UNS
    assert run(0, n, y, 16, None) == UNS
    assert run(48, n, y48, 48, None, tp=None) == UNS                                # the width comes first
    assert run(16, n, y, 12, None) == INV                                          # a stride of H - 4
    assert run(16, n, y, 18, None) == INV                                          # row stride no multiple of 4
    assert run(16, n, y, 16, None, base=TP._hip().ptr(y.view(-1)[1:])) == INV      # base not 16-byte aligned
    assert run(16, -1, y, 16, None) == INV
    assert run(16, 2 ** 31, y, 16, None) == INV
    assert run(16, n, y, 16, [0, 10, n - 1]) == INV                                # does not end at N
    assert run(16, n, y, 16, [1, 10, n]) == INV                                    # does not start at 0
    assert run(16, n, y, 16, None, tp=None) == INV                                 # NULL thr_ptr
    bad = good_tp.clone()
    bad[0] = 1
    assert run(16, n, y, 16, None, tp=bad) == INV                                  # does not start at 0
    bad = good_tp.clone()
    bad[-1] = -5
    assert run(16, n, y, 16, None, tp=bad) == INV                                  # T < 0
    assert run(16, n, y, 16, None, gt=False) == INV
    assert run(16, n, y, 16, None, eq=False) == INV
    assert run(16, n, y, 16, None, th=None) == INV
    zero = torch.zeros(n + 1, dtype=I32, device=dev)
    assert run(16, n, y, 16, None, tp=zero, gt=False, eq=False, th=None) == (0, True)     # T = 0: nothing to write, nothing launched
    assert run(16, 0, y, 16, None, tp=zero) == (0, True)                           # N = 0
    assert run(16, 0, y, 16, [0, 0], tp=zero) == (0, True)
    assert run(16, n, y, 16, [0, 10, n]) == (0, False)
    from deepgate import _hip, ops
    with pytest.raises(_hip.HipLibraryError, match='EINVAL'):
        ops.pair_rank_counts(y, y, good_tp, thr, graph_ptr=[0, 10, n - 1])
    with pytest.raises(_hip.HipLibraryError, match='EUNSUPPORTED'):
        ops.pair_rank_counts(y48, y48, good_tp, thr)
    with pytest.raises(_hip.HipLibraryError, match='N \\+ 1'):
        ops.pair_rank_counts(y, y, good_tp[:-1], thr)


# ------------------------------------------------------------------------------------------------ surface
def _same(ranks, ref):
    lo, hi, valid = ref
    return (np.array_equal(ranks.rank_lo.cpu().numpy(), lo) and np.array_equal(ranks.rank_hi.cpu().numpy(), hi)
            and np.array_equal(ranks.valid.cpu().numpy(), valid))


def _metrics_same(m, want):
    ok = all(np.array_equal(getattr(m, k).cpu().numpy(), want[k]) for k in ('ranked', 'hits_lo', 'hits_hi', 'sum_lo', 'sum_hi'))
    got, ref = m.mrr.cpu().numpy(), want['mrr']
    fin = ~np.isnan(ref)
    return ok and np.array_equal(np.isnan(got), ~fin) and bool((np.abs(got[fin] - ref[fin]) <= 1e-12 * np.abs(ref[fin])).all())


@pytest.mark.parametrize('H', HS)
def test_link_ranks_and_rank_metrics_against_the_definition(H):
    """topk_case (eight graphs, ties planted across a tile edge) with three links per node, a link that leaves its graph, self loops
    and a NaN row; both `by`, both `filtered`, skip_self on and off; the shuffled order; the plan's row pointers."""
    dev = _dev()
    import deepgate
    from deepgate import ops
    from deepgate.graph_plan import GraphPlan
    c = PR.topk_case(H, 1)
    gp, N = c['graph_ptr'], c['N']
    s, t = c['s'].clone(), c['t'].clone()
    s[100] = NAN
    walk = Walk(dev, s, t, gp)
    sd, td = s.to(dev), t.to(dev)
    ei = torch.unique(torch.cat([PR.edges_case(c, 3, 1), torch.tensor([[0, 200], [3, 10]])], 1), dim=1)
    ei = ei[:, torch.randperm(ei.shape[1], generator=torch.Generator().manual_seed(1))]
    eid = ei.to(dev)
    dec = deepgate.digae_layer.DirectedInnerProductDecoder()
    gae = deepgate.digae_model.DirectedGAE(encoder=None, decoder=dec)
    plan = GraphPlan(eid, N)
    n = 0
    for by in ('src', 'dst'):
        for filt in (True, False):
            for skip in (False, True):
                want = RR.link_ranks_ref(walk.dense, ei, gp, by, skip, filt)
                got = ops.link_ranks(sd, td, eid, graph_ptr=gp, by=by, skip_self=skip, filtered=filt)
                assert got.rank_lo.dtype == I64 and got.rank_lo.is_cuda and _same(got, want), (H, by, filt, skip)
                assert _same(ops.link_ranks(sd, td, eid, graph_ptr=gp, by=by, skip_self=skip, filtered=filt, plan=plan), want)
                assert _same(dec.rank(sd, td, eid, graph_ptr=gp, by=by, skip_self=skip, filtered=filt), want)
                n += int(want[2].sum())
            want = RR.link_ranks_ref(walk.dense, ei, gp, by, False, filt)
            wm = RR.rank_metrics_ref(*want, ei, gp, (1, 3, 10, 50), by)
            m, ranks = gae.link_ranking(sd, td, eid, gp, by=by, filtered=filt)
            assert _same(ranks, want) and _metrics_same(m, wm) and m.mrr.dtype == F64 and m.hits_lo.shape == (len(gp) - 1, 4)
            m2 = ops.rank_metrics(ranks, eid, gp, by=by)
            assert torch.equal(m2.mrr.view(I64), m.mrr.view(I64))                      # the same bits from run to run
    assert not want[2].all() and want[2].sum() > 1000
    z = ops.link_ranks(sd, td, eid[:, :0], graph_ptr=gp)
    assert z.rank_lo.shape == (0,) and z.valid.dtype == torch.bool
    with pytest.raises(ValueError, match='twice'):
        ops.link_ranks(sd, td, torch.cat([eid, eid[:, 7:8]], 1), graph_ptr=gp)
    with pytest.raises(ValueError, match='outside'):
        ops.link_ranks(sd, td, torch.tensor([[0], [N]], device=dev), graph_ptr=gp)
    print('RANK ops H=%d | %d links, %d ranks compared | ok' % (H, ei.shape[1], n))


def test_the_model_method_on_a_two_graph_batch():
    dev = _dev()
    import deepgate
    from deepgate import ops, synthetic as syn
    H = 64
    torch.manual_seed(0)
    enc = deepgate.digae_layer.DirectMultiGCNEncoder(dim_feature=6, dim_hidden=H, s_rounds=1, t_rounds=1, layernorm=True)
    model = deepgate.dg_ae_model_aig.Model(struct_encoder=enc, dim_hidden=H).to(dev).eval()
    graphs = [syn.make_graph('aig', 300, 12, 70 + i, n_inputs=24) for i in range(2)]
    batch = deepgate.CircuitBatch.from_arrays(syn.collate(graphs), device=dev)
    with torch.no_grad():
        hs, _ = model(batch)
    gp = batch.graph_ptr.tolist()
    assert gp == [0, 300, 600]
    s, t = model._decoder_halves(hs)
    dense = ops.pair_scores(s, t, sigmoid=False).detach().cpu().numpy()
    ei = batch.edge_index.cpu()
    for by, filt in (('dst', True), ('dst', False), ('src', True)):
        want = RR.link_ranks_ref(dense, ei, gp, by, False, filt)
        wm = RR.rank_metrics_ref(*want, ei, gp, (1, 10), by)
        for plan in (None, getattr(batch, '_mgv_plan', None)):
            m, ranks = model.link_ranking(hs, batch.edge_index, batch.graph_ptr, ks=(1, 10), by=by, filtered=filt, plan=plan)
            assert _same(ranks, want) and _metrics_same(m, wm)
    m, _ = model.link_ranking(hs, batch.edge_index, batch.graph_ptr)                  # the defaults: by target, filtered, four Ks
    assert m.hits_lo.shape == (2, 4) and m.ranked.tolist() == [int((ei[1] < 300).sum()), int((ei[1] >= 300).sum())]
    print('RANK model | MRR by target per graph: %s' % ', '.join('%.6f' % x for x in m.mrr.tolist()))


def test_feature_extract_prints_the_ranking(tmp_path, capsys):
    """examples/feature_extract.py --link_ranking 1,10: one line per circuit, and nothing new in the file."""
    _dev()
    import importlib
    from conftest import PKG_PARENT
    sys.path.insert(0, os.path.join(PKG_PARENT, 'examples'))
    fe = importlib.import_module('feature_extract')
    out = tmp_path / 'emb.npz'
    fe.main(['--type', 'aig', '--synthetic', '2', '--rounds', '1', '--batch_size', '2', '--link_ranking', '1,10', '--out', str(out)])
    text = capsys.readouterr().out
    rows = re.findall(r'\[INFO\] (\S+): link ranking by target: (\d+) links ranked, MRR ([\d.]+), Hits@1 ([\d.]+)\.\.([\d.]+) '
                      r'Hits@10 ([\d.]+)\.\.([\d.]+), mean rank ([\d.]+)\.\.([\d.]+)', text)
    assert [r[0] for r in rows] == ['graph0', 'graph1'], text
    for r in rows:
        n, mrr, h1a, h1b, h10a, h10b, mlo, mhi = int(r[1]), *[float(x) for x in r[2:]]
        assert n > 1000 and 0 < mrr <= 1 and 0 <= h1a <= h1b <= h10b <= 1 and h10a <= h10b and 1 <= mlo <= mhi <= 1024
    assert sorted(np.load(out).files) == sorted('graph%d/%s' % (i, k) for i in range(2) for k in ('hs', 'hf'))
