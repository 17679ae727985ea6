"""The two further consumers of the cross walk of csrc/pair_scores.hip — mgv_cross_union (classes without a pair list) and mgv_cross_hist
(the distribution of cross cosines) — through the C ABI and through the surface (ops.cross_classes(route='walk'), ops.cross_profile,
ops.cross_threshold_for), against tests/cross_walk_ref.py (pinned on the CPU by tests/test_cross_walk_spec.py).

Shapes: cross_match_ref.match_case (365 nodes in graphs of (70, 1, 64, 129, 0, 63, 5, 33), both peer tables, ties across the column-tile
borders 192 and 256, zero rows, a NaN row) and cross_walk_ref.small_case (64 graphs of 8 nodes under a random involution: one row tile
holds eight graphs whose peers lie in other column tiles); H = 16 / 32 / 64 / 128; thresholds 0.999, 0.25 and -2.0.
Exact, without a tolerance: the references are applied to the bits the EXISTING mgv_pair_scores_at reports for the device's own unit
rows, and labels, bins and counts are compared as integers.  Every array a kernel writes has guard words on both sides."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cross_match_ref as CR  # noqa: E402
import cross_walk_ref as WR  # noqa: E402
import test_hip_cross_match as XM  # noqa: E402  (_rows: the case and the device's unit rows of it; _tables)
import test_hip_embed_sim as ES  # noqa: E402  (_unit: mgv_row_unit on a strided operand)
import test_hip_pair_scores as TP  # noqa: E402

pytestmark = pytest.mark.gpu

F32, I32, I64 = torch.float32, torch.int32, torch.int64
HS = (16, 32, 64, 128)
CASES = tuple(sorted(CR.PEERS)) + ('small',)
GUARD, GARBAGE = 64, 123456789
MGV_EINVAL, MGV_EUNSUPPORTED = -1, -2
_dev, _ptr, _rc, _call, _slice = TP._dev, TP._ptr, TP._rc, TP._call, TP._slice


class Guarded:
    """A flat array of n entries with GUARD words of `fill` on both sides; v is the part a kernel may write, filled with `fill` too."""

    def __init__(self, n, dtype, dev, fill=GARBAGE):
        self.n, self.fill = n, fill
        self.buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
        self.v = self.buf[GUARD:GUARD + n]

    def intact(self):
        return bool((self.buf[:GUARD] == self.fill).all()) and bool((self.buf[GUARD + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.buf == self.fill).all())


@functools.lru_cache(maxsize=None)
def _case(H, name):
    """{'x', 'y' (the device's unit rows, on the host), 'gp', 'peer', 'N', 'G', 's'}: s float32 [N, N] holds the bits of
    mgv_pair_scores_at(y, y, sigmoid = 0) at every cross candidate [u, v] and every own-graph pair v > u, NaN elsewhere."""
    dev = _dev()
    if name == 'small':
        c = WR.small_case(H)
        x, gp, peer = c['x'], c['graph_ptr'].tolist(), c['peer'].tolist()
        y = ES._unit(dev, torch.from_numpy(x), want_norm=False)[0].v.cpu().contiguous()
    else:
        c, y = XM._rows(H)
        x, gp, peer = c['x'], XM.GP, list(CR.PEERS[name])
    N = gp[-1]
    graph_of = np.searchsorted(np.asarray(gp[1:]), np.arange(N), side='right')
    own = (graph_of[:, None] == graph_of[None, :]) & (np.arange(N)[None, :] > np.arange(N)[:, None])
    u, v = np.nonzero(CR.candidate_mask(gp, peer) | own)
    src, dst = torch.from_numpy(u).to(dev), torch.from_numpy(v).to(dev)
    yv, ldy = _slice(y, dev)
    out = TP.Out(u.size, 1, dev)
    _call('mgv_pair_scores_at', H, u.size, _ptr(yv), ldy, _ptr(yv), ldy, _ptr(src), _ptr(dst), 0, _ptr(out.v))
    assert out.intact()
    s = np.full((N, N), np.nan, dtype=np.float32)
    s[u, v] = out.v.flatten().cpu().numpy()
    return {'x': x, 'y': y, 'gp': gp, 'peer': peer, 'N': N, 'G': len(gp) - 1, 's': s, 'graph_of': graph_of}


def _operands(dev, c, peer=None):
    yv, ldy = _slice(c['y'], dev)
    gpd, prd = XM._tables(dev, c['peer'] if peer is None else peer, c['gp'])
    return (c['y'].shape[1], c['N'], _ptr(yv), ldy, _ptr(gpd), c['G'], _ptr(prd)), (yv, gpd, prd)


def _union(dev, c, thr, with_own, peer=None):
    """mgv_cc_init [+ mgv_sim_union] + mgv_cross_union + mgv_cc_labels on guarded arrays -> (label on the host, status, guards intact)."""
    args, keep = _operands(dev, c, peer)
    H, N = args[0], args[1]
    parent, status, label = Guarded(N, I32, dev), Guarded(4, I32, dev), Guarded(N, I32, dev)
    _call('mgv_cc_init', N, _ptr(parent.v), _ptr(status.v))
    if with_own:
        _call('mgv_sim_union', *args[:6], float(thr), _ptr(parent.v), _ptr(status.v))
    _call('mgv_cross_union', *args, float(thr), _ptr(parent.v), _ptr(status.v))
    _call('mgv_cc_labels', N, _ptr(parent.v), _ptr(label.v), None)
    return label.v.cpu(), status.v.tolist(), parent.intact() and status.intact() and label.intact()


def _hist(dev, c, edges):
    """mgv_cross_hist into a guarded hist prefilled with garbage -> (int64 [G, B + 1] on the host, guards intact)."""
    args, keep = _operands(dev, c)
    e = torch.as_tensor(np.asarray(edges, dtype=np.float32)).to(dev)
    h = Guarded(c['G'] * (e.numel() + 1), I64, dev)
    _call('mgv_cross_hist', *args, _ptr(e), e.numel(), _ptr(h.v))
    return h.v.cpu().view(c['G'], e.numel() + 1), h.intact()


def _n_sel(dev, c, thr):
    args, keep = _operands(dev, c)
    n_sel = Guarded(c['N'], I32, dev)
    _call('mgv_cross_select_count', *args, float(thr), _ptr(n_sel.v))
    assert n_sel.intact()
    return n_sel.v.cpu().to(I64)


def _per_graph(c, per_row):
    gp = c['gp']
    return torch.stack([per_row[gp[g]:gp[g + 1]].sum() for g in range(c['G'])])


# ------------------------------------------------------------------------------------------------ union
@pytest.mark.parametrize('name', CASES)
@pytest.mark.parametrize('H', HS)
def test_union_gives_the_components_of_the_lists(H, name):
    dev = _dev()
    from deepgate import ops
    c = _case(H, name)
    gp, peer, N, s = c['gp'], c['peer'], c['N'], c['s']
    xd = torch.from_numpy(c['x']).to(dev)
    info = CR.match_case(H)['info'] if name != 'small' else None
    bad, classes = [], []
    for thr in CR.THRESHOLDS:
        tag = 'H=%d %s thr=%g' % (H, name, thr)
        # the cross links alone
        label, status, intact = _union(dev, c, thr, False)
        want = torch.from_numpy(WR.classes_ref(s, gp, peer, thr, False))
        if not torch.equal(label.to(I64), want):
            bad.append('%s: cross labels differ from classes_ref in %d nodes' % (tag, int((label.to(I64) != want).sum())))
        comp = ops.components(ops.cross_pairs(xd, gp, peer, threshold=thr)[0], N)
        if not torch.equal(label, comp.cpu()):
            bad.append('%s: cross labels differ from ops.components(cross_pairs)' % tag)
        if status != [0, 0, 0, 0] or not intact:
            bad.append('%s: status %s, guards intact %s' % (tag, status, intact))
        again = _union(dev, c, thr, False)[0]
        if not torch.equal(label, again):
            bad.append('%s: a second run gives other labels' % tag)
        # own-graph links first, on the same forest
        both, status, intact = _union(dev, c, thr, True)
        want = torch.from_numpy(WR.classes_ref(s, gp, peer, thr, True))
        if not torch.equal(both.to(I64), want):
            bad.append('%s: labels of both walks differ from classes_ref in %d nodes' % (tag, int((both.to(I64) != want).sum())))
        if status != [0, 0, 0, 0] or not intact:
            bad.append('%s: both walks: status %s, guards intact %s' % (tag, status, intact))
        if not torch.equal(both, _union(dev, c, thr, True)[0]):
            bad.append('%s: both walks: a second run gives other labels' % tag)
        for min_size in (2, 1):
            via_pairs = ops.cross_classes(xd, gp, peer, threshold=thr, min_size=min_size, route='pairs')
            via_walk = ops.cross_classes(xd, gp, peer, threshold=thr, min_size=min_size, route='walk')
            if not torch.equal(both, via_pairs[0].cpu()):
                bad.append('%s: labels of both walks differ from cross_classes(route=pairs)' % tag)
            if not all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(via_walk, via_pairs)):
                bad.append('%s min_size=%d: route=walk and route=pairs return different tensors' % (tag, min_size))
        classes.append(int((both == torch.arange(N)).sum()))
        if info is not None and thr >= 0:
            for z in info['zeros'] + (info['nan'],):
                if int(both[z]) != z or int((both == z).sum()) != 1:
                    bad.append('%s: row %d (a zero row or the NaN row) is no singleton' % (tag, z))
    if name != 'small':
        # a graph whose peer is -1 and that nobody names joins nobody through a cross link: only the self-peer graph 5 has links here
        alone = [-1] * c['G']
        alone[5] = 5
        label, status, intact = _union(dev, c, -2.0, False, peer=alone)
        want = torch.from_numpy(WR.classes_ref(s if name == 'involution' else _case(H, 'involution')['s'], gp, alone, -2.0, False))
        out5 = torch.ones(N, dtype=torch.bool)
        out5[gp[5]:gp[6]] = False
        if not (torch.equal(label.to(I64), want) and bool((label[out5] == torch.arange(N)[out5]).all()) and status == [0, 0, 0, 0] and intact):
            bad.append('H=%d: with peer = -1 everywhere but the self-peer, a row outside it joined somebody' % H)
        if int((label[gp[5]:gp[6]] == gp[5]).sum()) < gp[6] - gp[5] - 2:      # below every cosine the self-peer graph is one class
            bad.append('H=%d: the self-peer graph is not one class at -2.0' % H)
    print('XW union H=%d %s | classes per threshold %s of %d nodes | %d findings' % (H, name, classes, N, len(bad)))
    assert not bad, bad[:10]


# ------------------------------------------------------------------------------------------------ histogram
def _edge_tables(c, name):
    s, gp, peer = c['s'], c['gp'], c['peer']
    if name == 'small':
        g = next(g for g in range(c['G']) if g < peer[g])
        tie = s[gp[g], gp[peer[g]]]
    else:
        info = CR.match_case(c['y'].shape[1])['info']
        tie = s[info['copy'], info['trio'][0]]
    tie = np.float32(tie)
    assert 0.999 < tie < 1.5
    dn, up = np.nextafter(tie, np.float32(-2)), np.nextafter(tie, np.float32(2))
    return {'B=1': np.asarray([0.25], dtype=np.float32),
            'B=7 around the tie': np.asarray([-0.5, 0.0, 0.25, 0.9, dn, tie, up], dtype=np.float32),
            'B=256': np.linspace(-1.0, 1.01, 256).astype(np.float32),
            'infinite ends': np.asarray([-np.inf, -0.2, 0.3, np.inf], dtype=np.float32)}, tie


@pytest.mark.parametrize('name', CASES)
@pytest.mark.parametrize('H', HS)
def test_hist_equals_the_comparisons_themselves(H, name):
    dev = _dev()
    c = _case(H, name)
    gp, peer, s = c['gp'], c['peer'], c['s']
    tables, tie = _edge_tables(c, name)
    lo, hi = CR.row_ranges(gp, peer)
    nan_cols = (np.isnan(s) & CR.candidate_mask(gp, peer)).sum(1)
    totals = _per_graph(c, torch.from_numpy((hi - lo) - nan_cols))
    bad, seen = [], []
    for tname, e in tables.items():
        tag = 'H=%d %s %s' % (H, name, tname)
        hist, intact = _hist(dev, c, e)
        want = torch.from_numpy(WR.hist_ref(s, gp, peer, e))
        if not torch.equal(hist, want):
            bad.append('%s: hist differs from hist_ref in %d bins' % (tag, int((hist != want).sum())))
        if not intact:
            bad.append('%s: guard words changed' % tag)
        if not torch.equal(hist.sum(1), totals):
            bad.append('%s: a row total is not rows(g) x rows(peer[g]) minus the NaN candidates' % tag)
        above = hist[:, 1:].flip(1).cumsum(1).flip(1)
        for j in range(e.size):
            if not torch.equal(above[:, j], _per_graph(c, _n_sel(dev, c, e[j]))):
                bad.append('%s: the suffix sum at edge %d (%r) is not the count walk\'s total' % (tag, j, float(e[j])))
        if not torch.equal(hist, _hist(dev, c, e)[0]):
            bad.append('%s: a second run gives other bytes' % tag)
        for g, p in enumerate(peer):
            if (p < 0 or gp[g + 1] == gp[g]) and bool(hist[g].any()):
                bad.append('%s: graph %d has no candidates and a non-zero row' % (tag, g))
        seen.append(int(hist.sum()))
    # the tie's own cosine as an edge takes the tie out, its lower neighbour keeps it: bins 5 and 6 of the second table
    hist = _hist(dev, c, tables['B=7 around the tie'])[0]
    ties = int(((s == tie) & CR.candidate_mask(gp, peer)).sum())
    if int(hist[:, 5].sum()) != ties or ties < 2:
        bad.append('H=%d %s: the bin between the tie\'s lower neighbour and the tie holds %d of %d tied pairs' % (H, name, int(hist[:, 5].sum()), ties))
    print('XW hist H=%d %s | candidates per table %s | %d tied pairs at %.9g | %d findings' % (H, name, seen, ties, float(tie), len(bad)))
    assert not bad, bad[:10]


def test_cross_profile_on_the_surface_is_the_abi():
    dev = _dev()
    from deepgate import ops
    from deepgate._model_base import FunctionalModel
    c = _case(64, 'involution')
    xd = torch.from_numpy(c['x']).to(dev)
    e = [-0.5, 0.25, 0.999]
    prof = ops.cross_profile(xd, e, c['gp'], c['peer'])
    assert prof.dtype == I64 and prof.shape == (c['G'], 4) and torch.equal(prof.cpu(), _hist(dev, c, e)[0])
    above = FunctionalModel.cross_similarity_profile(None, xd, e, c['gp'], c['peer'])
    assert torch.equal(above, ops.counts_above(prof))
    for j, thr in enumerate(e):
        row_ptr = ops.cross_pairs(xd, c['gp'], c['peer'], threshold=float(np.float32(thr)))[1].cpu()
        assert torch.equal(above[:, j].cpu(), _per_graph(c, row_ptr[1:] - row_ptr[:-1]))


# ------------------------------------------------------------------------------------------------ threshold by count
@pytest.mark.parametrize('name', CASES)
def test_threshold_for_is_the_lowest_threshold_that_fits(name):
    dev = _dev()
    from deepgate import ops
    H = 64
    c = _case(H, name)
    gp, peer, s = c['gp'], c['peer'], c['s']
    xd = torch.from_numpy(c['x']).to(dev)
    _, tie = _edge_tables(c, name)
    cand = s[CR.candidate_mask(gp, peer) & ~np.isnan(s)]
    group = int((cand == tie).sum())
    over = int((cand > tie).sum())
    at_quarter = int((cand > np.float32(0.25)).sum())
    assert group >= 2 and at_quarter > over + group
    # the counts a threshold t >= 0 can give: the count at 0 and the count above every value that occurs above 0
    values = np.unique(cand[cand > 0])
    steps = sorted({int((cand > np.float32(0)).sum())} | {int((cand > v).sum()) for v in values})
    seen = []
    for max_pairs in (0, over + group - 1, over + group, at_quarter):
        r = ops.cross_threshold_for(xd, max_pairs, gp, peer)
        total = ops.cross_pairs(xd, gp, peer, threshold=r['threshold'])[0].shape[1]
        print('XW threshold %s max_pairs=%d | %r | cross_pairs lists %d' % (name, max_pairs, r, total))
        assert r['pairs'] <= max_pairs and r['pairs'] == total and r['tight'] is True
        assert r['pairs'] == max(n for n in steps if n <= max_pairs)          # the LOWEST threshold that fits lists the most that fit
        if r['lower'] is not None:
            assert r['pairs_lower'] > max_pairs and r['lower'] < r['threshold']
            assert ops.cross_pairs(xd, gp, peer, threshold=r['lower'])[0].shape[1] == r['pairs_lower']
        seen.append(r['pairs'])
    assert seen[0] == 0 and seen[1] <= over and seen[2] == over + group      # the tie is taken or left as a whole
    from deepgate._model_base import FunctionalModel
    assert FunctionalModel.cross_equivalence_threshold(None, xd, over + group, gp, peer) == ops.cross_threshold_for(xd, over + group, gp, peer)
    with pytest.raises(ops.HipLibraryError, match='max_pairs'):
        ops.cross_threshold_for(xd, -1, gp, peer)


def test_feature_extract_cross_classes_and_cross_equivalences_max(tmp_path, capsys):
    """examples/feature_extract.py --cross_classes THR --cross_equivalences_max P on one batch of three circuits (a couple and an odd last
    graph): name/xcl_label local to the couple, name/xeq_threshold, at most P pairs in the batch's lists."""
    _dev()
    import importlib

    from conftest import PKG_PARENT
    sys.path.insert(0, os.path.join(PKG_PARENT, 'examples'))
    fe = importlib.import_module('feature_extract')
    out, P = tmp_path / 'emb.npz', 300
    fe.main(['--type', 'aig', '--synthetic', '3', '--rounds', '1', '--batch_size', '3', '--cross_classes', '0.999', '--cross_equivalences_max',
             str(P), '--out', str(out)])
    emb = np.load(out)
    assert sorted(emb.files) == sorted('graph%d/%s' % (i, k) for i in range(3) for k in ('hs', 'hf', 'xcl_label', 'xeq_pairs', 'xeq_cos',
                                                                                       'xeq_threshold'))
    n = [emb['graph%d/hf' % i].shape[0] for i in range(3)]
    thr = {float(emb['graph%d/xeq_threshold' % i]) for i in range(3)}
    assert len(thr) == 1 and 0.0 <= min(thr) <= 2.0
    assert sum(emb['graph%d/xeq_pairs' % i].shape[1] for i in range(3)) <= P and emb['graph2/xeq_pairs'].shape[1] == 0
    for i in range(3):
        assert bool((emb['graph%d/xeq_cos' % i] > min(thr)).all())
    l0, l1, l2 = (emb['graph%d/xcl_label' % i] for i in range(3))
    assert l0.dtype == np.int32 and l0.shape == (n[0],) and l1.shape == (n[1],) and l2.shape == (n[2],)
    assert (l0 <= np.arange(n[0])).all() and (l0 >= 0).all()                  # graph 0 comes first in its couple: labels are its own gates
    assert (l1 <= n[0] + np.arange(n[1])).all() and (l1 >= 0).all()           # graph 1: a label below n[0] is a gate of graph 0
    assert (l2 <= np.arange(n[2])).all() and (l2 >= 0).all()                  # the odd last graph has no peer: local ids
    spanning = np.unique(l1[l1 < n[0]]).size
    text = capsys.readouterr().out
    assert 'graph0: %d classes hold gates of it and of graph 1 at cos(hf) > 0.999' % spanning in text


# ------------------------------------------------------------------------------------------------ the identity peer: the own-graph walk
def _own(H):
    """match_case with peer[g] = g: every row's candidates are the rows of its own graph, itself included."""
    c = _case(H, 'involution')
    return dict(c, peer=list(range(c['G'])))


@pytest.mark.parametrize('H', HS)
def test_hist_under_the_identity_peer_is_the_own_graph_hist(H):
    """mgv_cross_hist with peer[g] = g against mgv_pair_hist(y, y, sigmoid = 0, skip_self = 0) on the same unit rows and edges, entry for
    entry; tables of 1, 64 and 256 edges: a search of 1, 7 and 9 steps."""
    dev = _dev()
    c = _own(H)
    (Hh, N, y, ldy, gpd, G, _), keep = _operands(dev, c)
    for B in (1, 64, 256):
        edges = np.asarray([0.25], dtype=np.float32) if B == 1 else np.linspace(-1.0, 1.01, B).astype(np.float32)
        cross, intact = _hist(dev, c, edges)
        e = torch.from_numpy(edges).to(dev)
        h = Guarded(G * (B + 1), I64, dev)
        _call('mgv_pair_hist', Hh, N, y, ldy, y, ldy, gpd, G, 0, 0, _ptr(e), B, _ptr(h.v))
        own = h.v.cpu().view(G, B + 1)
        print('XW identity hist H=%d B=%d | %d candidates | %d bins differ' % (H, B, int(own.sum()), int((cross != own).sum())))
        assert cross.dtype == I64 and torch.equal(cross, own) and intact and h.intact(), B
        assert int(own.sum()) > 0


@pytest.mark.parametrize('H', HS)
def test_union_under_the_identity_peer_gives_the_labels_of_the_own_graph_union(H):
    """mgv_cross_union with peer[g] = g on a fresh forest, then mgv_cc_labels, against mgv_sim_union: the cross walk meets every pair
    from both sides and the diagonal besides, and the components are the same."""
    dev = _dev()
    c = _own(H)
    args, keep = _operands(dev, c)
    N = c['N']
    for thr in (0.999, 0.25):
        cross, status, intact = _union(dev, c, thr, False)
        parent, st, label = Guarded(N, I32, dev), Guarded(4, I32, dev), Guarded(N, I32, dev)
        _call('mgv_cc_init', N, _ptr(parent.v), _ptr(st.v))
        _call('mgv_sim_union', *args[:6], float(thr), _ptr(parent.v), _ptr(st.v))
        _call('mgv_cc_labels', N, _ptr(parent.v), _ptr(label.v), None)
        own = label.v.cpu()
        classes = int((own == torch.arange(N)).sum())
        print('XW identity union H=%d thr=%g | %d classes of %d nodes | %d labels differ' % (H, thr, classes, N, int((cross != own).sum())))
        assert torch.equal(cross, own) and status == [0, 0, 0, 0] and st.v.tolist() == [0, 0, 0, 0], thr
        assert intact and parent.intact() and st.intact() and label.intact()
        assert classes < N                                  # the threshold unites somebody: the case has copies


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_are_return_codes_before_anything_is_launched_or_zeroed():
    dev = _dev()
    n, B = 40, 3
    y48, y = torch.randn(n, 48, device=dev), torch.randn(n, 16, device=dev)
    gp, peer = [0, 10, n], [1, 0]
    good_edges = [-0.5, 0.0, 0.5]

    def both(H, nn, x, ld, gp, peer, edges=good_edges, nulls=(), Bn=None):
        """(mgv_cross_union's code, mgv_cross_hist's code, forest as mgv_cc_init left it, hist untouched); the union runs below every
        cosine, so a launch changes the forest"""
        parent, status = Guarded(n, I32, dev), Guarded(4, I32, dev)
        _call('mgv_cc_init', n, _ptr(parent.v), _ptr(status.v))
        fresh = (parent.buf.clone(), status.buf.clone())
        gpd = None if gp is None else torch.tensor(gp, dtype=I32, device=dev)
        prd = None if peer is None else torch.tensor(peer, dtype=I32, device=dev)
        Gn = 0 if gp is None else len(gp) - 1
        e = torch.tensor(edges, dtype=F32, device=dev)
        h = Guarded(max(Gn, 1) * 257, I64, dev)
        common = (H, nn, _ptr(x), ld, _ptr(gpd), Gn, _ptr(prd))
        a = _rc('mgv_cross_union', *common, -2.0, None if 'parent' in nulls else _ptr(parent.v), None if 'status' in nulls else _ptr(status.v))
        b = _rc('mgv_cross_hist', *common, None if 'edges' in nulls else _ptr(e), len(edges) if Bn is None else Bn,
                None if 'hist' in nulls else _ptr(h.v))
        assert status.v.tolist() == [0, 0, 0, 0]
        return a, b, torch.equal(parent.buf, fresh[0]) and torch.equal(status.buf, fresh[1]), h.untouched()
    U, E = MGV_EUNSUPPORTED, MGV_EINVAL
    assert both(48, n, y48, 48, gp, peer) == (U, U, True, True)                    # bad H
    assert both(0, n, y, 16, gp, peer) == (U, U, True, True)
    assert both(16, n, y, 16, gp, None) == (E, E, True, True)                      # a NULL peer
    assert both(16, n, y, 16, None, peer) == (E, E, True, True)                    # a NULL graph_ptr
    assert both(16, n, y, 16, gp, [1, 2]) == (E, E, True, True)                    # a peer entry equal to G
    assert both(16, n, y, 16, gp, [-2, 0]) == (E, E, True, True)
    assert both(16, n, y, 16, gp, peer, nulls=('parent',)) == (E, 0, True, False)
    assert both(16, n, y, 16, gp, peer, nulls=('status',)) == (E, 0, True, False)
    assert both(16, n, y, 16, gp, peer, nulls=('edges',)) == (0, E, False, True)
    assert both(16, n, y, 16, gp, peer, nulls=('hist',)) == (0, E, False, True)
    assert both(16, n, y, 16, gp, peer, Bn=0)[1::2] == (E, True)                   # B outside 1 .. 256
    assert both(16, n, y, 16, gp, peer, edges=[0.0] * 257)[1::2] == (E, True)
    assert both(16, n, y, 16, gp, peer, edges=[0.0, 0.5, 0.5])[1::2] == (E, True)  # a table that does not ascend strictly
    assert both(16, n, y, 16, gp, peer, edges=[0.5, 0.0, 0.7])[1::2] == (E, True)
    assert both(16, n, y, 16, gp, peer, edges=[0.0, float('nan'), 0.7])[1::2] == (E, True)
    assert both(16, n, y, 16, gp, peer, edges=[float('nan')])[1::2] == (E, True)
    assert both(16, n, y, 12, gp, peer) == (E, E, True, True)                      # row stride below H
    assert both(16, n, y, 16, [0, 10, n - 1], peer) == (E, E, True, True)          # graph_ptr does not end at N
    assert both(16, -1, y, 16, gp, peer) == (E, E, True, True)
    assert both(16, n, y, 16, gp, peer) == (0, 0, False, False)
    # N = 0 succeeds: hist is zeroed, the forest is not touched
    empty = torch.full((1, 16), float('nan'), device=dev)
    parent, status, h = Guarded(n, I32, dev), Guarded(4, I32, dev), Guarded(2 * (B + 1), I64, dev)
    gpd, prd, e = torch.tensor([0, 0, 0], dtype=I32, device=dev), torch.tensor([1, 0], dtype=I32, device=dev), torch.tensor(good_edges, device=dev)
    common = (16, 0, _ptr(empty), 16, _ptr(gpd), 2, _ptr(prd))
    assert _rc('mgv_cross_union', *common, 0.5, _ptr(parent.v), _ptr(status.v)) == 0 and parent.untouched() and status.untouched()
    assert _rc('mgv_cross_hist', *common, _ptr(e), B, _ptr(h.v)) == 0 and h.intact() and not bool(h.v.any())
    from deepgate import _hip, ops
    with pytest.raises(_hip.HipLibraryError, match='EUNSUPPORTED'):
        ops.cross_classes(y48, gp, peer, route='walk')
    with pytest.raises(_hip.HipLibraryError, match='EUNSUPPORTED'):
        ops.cross_profile(y48, good_edges, gp, peer)
    with pytest.raises(_hip.HipLibraryError, match='EINVAL'):
        ops.cross_profile(y, [0.5, 0.5], gp, peer)
    label, class_ptr, members = ops.cross_classes(torch.zeros(0, 16, device=dev), [0, 0], [0], route='walk')
    assert label.shape == (0,) and class_ptr.tolist() == [0] and members.shape == (0,)
    assert ops.cross_profile(torch.zeros(0, 16, device=dev), good_edges, [0, 0], [0]).tolist() == [[0, 0, 0, 0]]
