"""tests/cross_walk_ref.py pinned on the CPU: classes_ref against a brute-force BFS on the dense boolean relation, hist_ref's suffix sums
against select_ref's row counts; the header's two new entries and their reference lines; the host's refusals of ops.cross_classes
(route, max_pairs with the walk, a bad peer) before anything touches the device; the surface."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cross_match_ref as CR  # noqa: E402
import cross_walk_ref as WR  # noqa: E402


def _cos64(x):
    y = CR.unit_rows64(x)
    return y @ y.T


def _bfs_labels(rel):
    """label[i] = the smallest id reachable from i in the undirected graph of the boolean matrix rel (either direction links)."""
    n = rel.shape[0]
    sym = rel | rel.T
    nbr = [np.nonzero(sym[i])[0].tolist() for i in range(n)]
    label = [-1] * n
    for root in range(n):
        if label[root] >= 0:
            continue
        label[root] = root
        queue = [root]
        while queue:
            i = queue.pop()
            for j in nbr[i]:
                if label[j] < 0:
                    label[j] = root
                    queue.append(j)
    return np.asarray(label, dtype=np.int64)


def _relation(score, gp, peer, thr, with_own):
    n = score.shape[0]
    with np.errstate(invalid='ignore'):
        rel = CR.candidate_mask(gp, peer) & (score > thr)
        if with_own:
            graph_of = np.searchsorted(np.asarray(gp)[1:], np.arange(n), side='right')
            rel = rel | ((graph_of[:, None] == graph_of[None, :]) & (np.arange(n)[None, :] > np.arange(n)[:, None]) & (score > thr))
    return rel


def _cases():
    out = [(c['x'], c['graph_ptr'], CR.PEERS[t]) for c in (CR.match_case(16), CR.match_case(64)) for t in sorted(CR.PEERS)]
    s = WR.small_case(32)
    return out + [(s['x'], s['graph_ptr'], s['peer'])]


def test_classes_ref_equals_a_bfs_on_the_dense_relation():
    spans_two = 0
    for x, gp, peer in _cases():
        cos = _cos64(x)
        graph_of = np.searchsorted(np.asarray(gp)[1:], np.arange(cos.shape[0]), side='right')
        for thr in CR.THRESHOLDS:
            for with_own in (False, True):
                got = WR.classes_ref(cos, gp, peer, thr, with_own)
                want = _bfs_labels(_relation(cos, gp, peer, thr, with_own))
                assert np.array_equal(got, want), (thr, with_own)
                assert np.array_equal(got[got], got) and (got <= np.arange(got.size)).all()
                spans_two += any(len(set(graph_of[got == r].tolist())) > 1 for r in np.unique(got))
    assert spans_two > 0


def test_the_planted_rows_of_the_case_are_singletons_or_joined_as_designed():
    c = CR.match_case(64)
    cos, gp, info = _cos64(c['x']), c['graph_ptr'], c['info']
    for table, peer in CR.PEERS.items():
        for thr in (0.999, 0.25):
            lab = WR.classes_ref(cos, gp, peer, thr, True)
            for z in info['zeros'] + (info['nan'],):
                assert lab[z] == z and int((lab == z).sum()) == 1, (table, thr, z)
        lab = WR.classes_ref(cos, gp, peer, 0.999, False)
        assert len({int(lab[v]) for v in info['trio'] + (info['half'], info['copy'], info['times4'])}) == 1      # graph 0 names graph 3
        none = [g for g, p in enumerate(peer) if p < 0 and gp[g + 1] > gp[g]]
        named = {p for p in peer if p >= 0}
        for g in none:
            if g not in named:                              # nobody names it either: its rows stay alone through cross links
                assert (lab[gp[g]:gp[g + 1]] == np.arange(gp[g], gp[g + 1])).all()


def test_small_case_has_the_features_it_was_designed_for():
    s = WR.small_case(16)
    gp, peer = s['graph_ptr'], s['peer']
    assert s['N'] == 512 and peer.size == 64 and (peer[peer] == np.arange(64)).all() and (peer != np.arange(64)).all()
    lo, _ = CR.row_ranges(gp, peer)
    assert any(len({int(a) // 64 for a in lo[64 * t:64 * t + 64]}) >= 4 for t in range(8))      # one row tile, peers in many column tiles
    assert any(len(CR.tile_spans(gp, peer, t)) >= 2 for t in range(8))
    lab = WR.classes_ref(_cos64(s['x']), gp, peer, 0.999, True)
    sizes = np.bincount(lab, minlength=512)
    assert int((sizes >= 2).sum()) >= 2 * 32 + 16            # a class per couple's row 0 and row 1, one per fourth graph's rows 2 and 3


def test_hist_ref_suffix_sums_equal_select_ref_row_counts_per_graph():
    tables = {'one': [0.25], 'seven': [-0.5, 0.0, 0.25, 0.5, 0.9, 0.999, 1.5], 'wide': np.linspace(-1.0, 1.01, 256),
              'inf': [-np.inf, -0.2, 0.3, np.inf]}
    for x, gp, peer in _cases():
        cos = _cos64(x).astype(np.float32)
        lo, hi = CR.row_ranges(gp, peer)
        nan_cols = (np.isnan(cos) & CR.candidate_mask(gp, peer)).sum(1)
        G = len(gp) - 1
        for name, edges in tables.items():
            e = np.asarray(edges, dtype=np.float32)
            hist = WR.hist_ref(cos, gp, peer, e)
            assert hist.shape == (G, e.size + 1) and hist.dtype == np.int64 and (hist >= 0).all()
            above = WR.counts_above_ref(hist)
            assert above.shape == (G, e.size)
            for j in range(e.size):
                row_ptr, _, _ = CR.select_ref(cos, gp, peer, e[j])
                n_sel = np.diff(row_ptr)
                want = np.asarray([n_sel[gp[g]:gp[g + 1]].sum() for g in range(G)])
                assert np.array_equal(above[:, j], want), (name, j)
                assert np.array_equal(above[:, j], hist[:, j + 1:].sum(1))
            total = np.asarray([((hi - lo) - nan_cols)[gp[g]:gp[g + 1]].sum() for g in range(G)])
            assert np.array_equal(hist.sum(1), total), name
            for g, p in enumerate(peer):
                if p < 0 or gp[g + 1] == gp[g]:
                    assert not hist[g].any()
            if name == 'inf':
                assert not hist[:, 0].any() and not hist[:, -1].any()     # everything is above -inf, nothing above +inf


def test_the_header_declares_the_two_entries_with_their_reference_lines():
    from deepgate import _hip
    sigs = _hip.parse_header()
    assert len(sigs['mgv_cross_union']) == 11 and len(sigs['mgv_cross_hist']) == 11
    with open(_hip.HEADER_PATH) as f:
        text = f.read()
    for name in ('mgv_cross_union', 'mgv_cross_hist'):
        head = text[:text.index('int %s(' % name)]
        comment = head[head.rindex('/*'):]
        assert 'trainer.py:158-160' in comment and 'digae_layer.py:31-33' in comment
        assert 'MGV_EINVAL' in comment and 'mgv_cross_select_' in comment


def test_cross_classes_refuses_on_the_host_before_any_device_work():
    from deepgate import ops
    from deepgate._hip import HipLibraryError
    gp = CR.graph_ptr_of(CR.GRAPH_SIZES).tolist()
    good = list(CR.PEERS['involution'])
    x = torch.zeros(365, 16)                                  # on the CPU: a call that got past the refusals would fail otherwise
    with pytest.raises(HipLibraryError, match='route'):
        ops.cross_classes(x, gp, good, route='bogus')
    with pytest.raises(HipLibraryError, match='max_pairs'):
        ops.cross_classes(x, gp, good, route='walk', max_pairs=10)
    with pytest.raises(HipLibraryError, match='min_size'):
        ops.cross_classes(x, gp, good, route='walk', min_size=0)
    bad = {'short': good[:-1], 'G': good[:-1] + [8], 'below -1': [-2] + good[1:], 'float': [float(v) for v in good]}
    for route in ('walk', 'pairs'):
        for tag, pr in bad.items():
            with pytest.raises(ValueError):
                ops.cross_classes(x, gp, pr, route=route)
        with pytest.raises(HipLibraryError, match='graph_ptr'):
            ops.cross_classes(x, None, good, route=route)
    for f in (lambda pr, gpp: ops.cross_profile(x, [0.5], gpp, pr), lambda pr, gpp: ops.cross_threshold_for(x, 10, gpp, pr)):
        for tag, pr in bad.items():
            with pytest.raises(ValueError):
                f(pr, gp)
        with pytest.raises(HipLibraryError, match='graph_ptr'):
            f(good, None)


def test_the_surface_names_the_new_operators():
    from deepgate import ops, similarity
    from deepgate._model_base import FunctionalModel as M
    assert ops.cross_profile is similarity.cross_profile and ops.cross_threshold_for is similarity.cross_threshold_for
    p = inspect.signature(ops.cross_classes).parameters
    assert p['route'].default == 'pairs' and p['threshold'].default == 0.999 and p['max_pairs'].default is None
    assert list(inspect.signature(ops.cross_profile).parameters) == ['x', 'edges', 'graph_ptr', 'peer', 'eps']
    q = inspect.signature(ops.cross_threshold_for).parameters
    assert list(q) == ['x', 'max_pairs', 'graph_ptr', 'peer', 'lo', 'bins', 'max_rounds', 'eps']
    assert q['lo'].default == 0.0 and q['bins'].default == 64 and q['max_rounds'].default == 6 and q['eps'].default == 1e-8
    assert 'ONCE FROM EACH SIDE' in ops.cross_threshold_for.__doc__
    assert inspect.signature(M.cross_equivalence_classes).parameters['route'].default == 'pairs'
    assert list(inspect.signature(M.cross_similarity_profile).parameters) == ['self', 'hf', 'thresholds', 'graph_ptr', 'peer']
    assert list(inspect.signature(M.cross_equivalence_threshold).parameters) == ['self', 'hf', 'max_pairs', 'graph_ptr', 'peer', 'lo']
    for f in (M.cross_similarity_profile, M.cross_equivalence_threshold):
        doc = ' '.join(f.__doc__.split())
        assert 'Added functionality' in doc and 'peer' in doc and 'trainer.py:158-160' in doc
