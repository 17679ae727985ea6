"""tests/cross_match_ref.py pinned on the CPU: the restatement of the cross-circuit selections against a brute-force dense float64
product written a second, slower way; the designed features of the case builders the device tests rely on; the host's validation of
`peer` (deepgate.similarity._peer_table and the operators in front of which it stands); the header and the surface."""
import inspect
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cross_match_ref as CR  # noqa: E402

HS = (16, 32, 64, 128)


def _cos64(c):
    y = CR.unit_rows64(c['x'])
    return y @ y.T


def _brute(score, gp, peer, k, thr):
    """Plain Python, one pair at a time: the candidates of u, sorted with a key, cut and padded."""
    N = int(gp[-1])
    graph_of = [g for g in range(len(gp) - 1) for _ in range(int(gp[g + 1] - gp[g]))]
    idx, top, n_above, lists = [], [], [], []
    for u in range(N):
        p = peer[graph_of[u]]
        cand = [] if p < 0 else [v for v in range(int(gp[p]), int(gp[p + 1])) if not math.isnan(score[u][v])]
        best = sorted(cand, key=lambda v: (-score[u][v], v))[:k]
        idx.append(best + [-1] * (k - len(best)))
        top.append([score[u][v] for v in best] + [-math.inf] * (k - len(best)))
        above = [v for v in cand if score[u][v] > thr]
        n_above.append(len(above))
        lists.append(above)
    return idx, top, n_above, lists


@pytest.mark.parametrize('table', sorted(CR.PEERS))
def test_the_restatement_equals_a_brute_force_float64_product(table):
    peer = CR.PEERS[table]
    for H in (16, 64):
        c = CR.match_case(H)
        gp, cos = c['graph_ptr'], _cos64(c)
        rows = cos.tolist()
        for k in CR.KS:
            for thr in CR.THRESHOLDS:
                idx, top, n_above = CR.topk_ref(cos, gp, peer, k, thr)
                b_idx, b_top, b_above, b_lists = _brute(rows, gp, peer, k, thr)
                assert idx.tolist() == b_idx and n_above.tolist() == b_above
                assert np.array_equal(top, np.asarray(b_top))
                row_ptr, col, val = CR.select_ref(cos, gp, peer, thr)
                assert row_ptr.tolist() == [0] + np.cumsum(b_above).tolist()
                assert col.tolist() == [v for lst in b_lists for v in lst]
                assert np.array_equal(val, np.asarray([rows[u][v] for u, lst in enumerate(b_lists) for v in lst]))
                assert np.array_equal(np.diff(row_ptr), n_above)


def test_the_tables_have_the_features_they_were_designed_for():
    gp = CR.graph_ptr_of(CR.GRAPH_SIZES)
    sizes, G = list(CR.GRAPH_SIZES), len(CR.GRAPH_SIZES)
    assert int(gp[-1]) == 365 and 0 in sizes and 1 in sizes and CR.TILE in sizes and CR.TILE - 1 in sizes and 2 * CR.TILE + 1 in sizes
    # graph borders inside a 64-row tile, off a 16-row wave border, and a tile border inside a graph
    assert any(b % CR.TILE for b in gp[1:-1]) and any(b % CR.WAVE_ROWS for b in gp[1:-1])
    assert any(gp[g] // CR.TILE != (gp[g + 1] - 1) // CR.TILE for g in range(G) if sizes[g])
    assert max(CR.KS) == CR.HEAP and any(0 < n < max(CR.KS) for n in sizes) and any(n > max(CR.KS) for n in sizes)
    inv, many = CR.PEERS['involution'], CR.PEERS['many_to_one']
    for peer in (inv, many):
        assert len(peer) == G and all(-1 <= p < G for p in peer)
    assert all(p < 0 or inv[p] == g for g, p in enumerate(inv))                       # an involution
    assert any(p == g for g, p in enumerate(inv)) and inv[sizes.index(0)] == -1       # a self-peer; the empty graph names nobody
    assert any(p >= 0 and p != g and sizes[p] != sizes[g] for g, p in enumerate(inv))  # unequal sizes
    assert any(many.count(p) >= 3 for p in set(many) if p >= 0)                        # many to one
    assert any(p >= 0 and many[p] != g for g, p in enumerate(many))                    # not an involution
    assert -1 in many and many[sizes.index(0)] >= 0                                    # the empty graph names a peer: rows it does not have
    # row tiles whose rows name peers that lie apart: more than one graph in the tile, and, for the involution, a gap between two spans
    tiles = range((365 + CR.TILE - 1) // CR.TILE)
    assert any(len(CR.tile_spans(gp, inv, t)) >= 2 for t in tiles)
    lo, hi = CR.row_ranges(gp, many)
    assert any(len({(a, b) for a, b in zip(lo[64 * t:64 * t + 64], hi[64 * t:64 * t + 64]) if a < b}) >= 2 for t in tiles)
    for peer in (inv, many):
        for t in tiles:
            spans = CR.tile_spans(gp, peer, t)
            assert all(a < b for a, b in spans) and all(spans[i][1] < spans[i + 1][0] for i in range(len(spans) - 1))
            lo, hi = CR.row_ranges(gp, peer)
            need = {ct for a, b in zip(lo[64 * t:64 * t + 64], hi[64 * t:64 * t + 64]) for ct in range(a // 64, (b + 63) // 64) if a < b}
            assert need == {ct for a, b in spans for ct in range(a, b)}


@pytest.mark.parametrize('H', HS)
def test_the_case_holds_its_planted_rows(H):
    c = CR.match_case(H)
    x, gp, info = c['x'], c['graph_ptr'], c['info']
    assert x.shape == (365, H) and x.dtype == np.float32
    graph_of = np.searchsorted(gp[1:], np.arange(365), side='right')
    t0, t1, t2 = info['trio']
    assert {int(graph_of[v]) for v in info['trio'] + (info['half'],)} == {3} and graph_of[info['copy']] == graph_of[info['times4']] == 0
    assert t0 // 64 != t1 // 64 and t1 // 64 != t2 // 64                               # the ties lie across column-tile borders
    assert np.array_equal(x[t0], x[t1]) and np.array_equal(x[t0], x[t2]) and np.array_equal(x[info['half']] * 2, x[t0])
    assert np.array_equal(x[info['times4']], 4 * x[info['copy']]) and np.array_equal(x[info['copy']], x[t0])
    a, b = info['self_pair']
    assert graph_of[a] == graph_of[b] == 5 and np.array_equal(x[a], x[b])
    assert all(not x[z].any() for z in info['zeros']) and {int(graph_of[z]) for z in info['zeros']} == {0, 3, 5}
    nan_rows = np.nonzero(np.isnan(x).any(1))[0].tolist()
    assert nan_rows == [info['nan']] and int(np.isnan(x[info['nan']]).sum()) == 1
    s0, s1 = info['scaled']
    assert np.array_equal(x[s1], 8 * x[s0]) and graph_of[s0] == graph_of[s1] == 2
    # in float64 the planted rows are what they were planted for, under both tables
    cos = _cos64(c)
    for peer in CR.PEERS.values():
        idx, top, n_above = CR.topk_ref(cos, gp, peer, 8, 0.999)
        for u in (info['copy'], info['times4']):
            assert idx[u, :4].tolist() == sorted(info['trio'] + (info['half'],)) and n_above[u] == 4
        z = info['zeros'][0]
        assert not top[z][idx[z] >= 0].any() and n_above[z] == 0
        assert not (idx == info['nan']).any()
        if peer[3] >= 0:
            assert (idx[info['nan']] == -1).all() and n_above[info['nan']] == 0
    idx, _, _ = CR.topk_ref(cos, gp, CR.PEERS['involution'], 2, 0.999)
    assert sorted(idx[a].tolist()) == [a, b] and idx[a, 0] == a                        # a self-peer: a row is its own candidate


def test_mutual_ref_on_a_table_small_enough_to_read():
    gp, peer = [0, 2, 4, 5], [1, 0, -1]
    idx1 = np.array([2, 3, 0, 0, -1])
    top1 = np.array([0.9, 0.95, 0.9, 0.8, -np.inf])
    pairs, cos = CR.mutual_ref(idx1, top1, gp, peer, 0.5)
    assert pairs.tolist() == [[0], [2]] and cos.tolist() == [0.9]                      # 1 -> 3 -> 0 is not reciprocal
    assert CR.mutual_ref(idx1, top1, gp, peer, 0.9)[0].shape == (2, 0)                # `>` is strict
    assert CR.mutual_ref(idx1, top1, gp, [1, 1, -1], 0.5)[0].shape == (2, 0)          # peer[peer[0]] != 0: nothing


# ------------------------------------------------------------------------------------------------ the host side
def test_peer_is_validated_on_the_host_before_anything_touches_the_device():
    from deepgate import ops, similarity
    from deepgate._hip import HipLibraryError
    gp = CR.graph_ptr_of(CR.GRAPH_SIZES).tolist()
    good = list(CR.PEERS['involution'])
    g, p = similarity._peer_table(good, gp, 'test')
    assert g.dtype == torch.int32 and p.dtype == torch.int32 and g.tolist() == gp and p.tolist() == good and not p.is_cuda
    assert similarity._peer_table(torch.tensor(good), torch.tensor(gp), 'test')[1].tolist() == good
    assert similarity._peer_table(np.asarray(good), np.asarray(gp), 'test')[1].tolist() == good
    assert similarity._peer_table([], [0], 'test')[1].numel() == 0
    x = torch.zeros(365, 16)                                  # on the CPU: a call that got past the validation would fail otherwise
    bad = {'short': good[:-1], 'long': good + [0], 'G': good[:-1] + [8], 'below -1': [-2] + good[1:], 'float': [float(v) for v in good],
           'bool': [True] * 8, '2-d': [good]}
    for f in (lambda pr, gpp: ops.cross_topk(x, 4, gpp, pr), lambda pr, gpp: ops.cross_pairs(x, gpp, pr),
              lambda pr, gpp: ops.cross_mutual(x, gpp, pr), lambda pr, gpp: ops.cross_classes(x, gpp, pr),
              lambda pr, gpp: similarity._peer_table(pr, gpp, 'test')):
        for tag, pr in bad.items():
            with pytest.raises(ValueError):
                f(pr, gp)
            with pytest.raises(ValueError):
                f(torch.tensor(pr), gp)
        with pytest.raises(HipLibraryError, match='graph_ptr'):
            f(good, None)
    with pytest.raises(HipLibraryError, match='min_size'):
        ops.cross_classes(x, gp, good, min_size=0)


def test_cross_room_refuses_like_sim_room():
    from deepgate import similarity
    from deepgate._hip import HipLibraryError
    with pytest.raises(HipLibraryError, match='max_pairs') as e:
        similarity._cross_room(11, False, 10, None)
    assert 'cross_pairs' in str(e.value) and 'cross_topk' in str(e.value) and '11' in str(e.value)
    with pytest.raises(HipLibraryError, match='GiB'):
        similarity._cross_room(2 ** 30, True, None, 2 ** 30)
    similarity._cross_room(10, True, 10, 240)
    similarity._cross_room(10, False, None, 200)


def test_the_header_declares_the_entries_and_the_surface_names_them():
    from deepgate import _hip, ops
    from deepgate._model_base import FunctionalModel as M
    sigs = _hip.parse_header()
    assert len(sigs['mgv_cross_topk']) == 13 and len(sigs['mgv_cross_select_count']) == 10 and len(sigs['mgv_cross_select_fill']) == 13
    with open(_hip.HEADER_PATH) as f:
        text = f.read()
    for name in ('mgv_cross_topk', 'mgv_cross_select_count', 'mgv_cross_select_fill'):
        head = text[:text.index('int %s(' % name)]
        comment = head[head.rindex('/*'):]
        assert 'trainer.py:158-160' in comment and 'digae_layer.py:31-33' in comment
    for f in (ops.cross_topk, ops.cross_pairs, ops.cross_mutual, ops.cross_classes):
        assert inspect.signature(f).parameters['threshold'].default == 0.999
        assert list(inspect.signature(f).parameters)[:1] == ['x'] and 'peer' in inspect.signature(f).parameters
    assert 'ONCE FROM EACH SIDE' in ops.cross_pairs.__doc__
    for f in (M.match_gates, M.cross_equivalence_candidates, M.cross_equivalence_classes):
        doc = ' '.join(f.__doc__.split())
        assert 'Added functionality' in doc and 'peer' in doc and inspect.signature(f).parameters['threshold'].default == 0.999
