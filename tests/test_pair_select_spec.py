"""CPU pins of tests/pair_select_ref.py, the reference and the checkers behind tests/test_hip_pair_select.py (mgv_pair_select_count /
mgv_pair_select_fill of csrc/pair_scores.hip): select_ref against the count references of pair_scores_ref, the properties of the case
builders the device tests rely on, the measured band around each threshold, planted defects of a restated fill against the checker the
device file uses, and the host-only paths of ops.pair_select."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_scores_ref as PR  # noqa: E402
import pair_select_ref as SR  # noqa: E402

F64, F32, I64 = torch.float64, torch.float32, torch.int64
HS = (16, 32, 64, 128)


@functools.lru_cache(maxsize=None)
def _case(H, seed=1, sizes=SR.SIZES):
    c = SR.select_case(H, seed, sizes=sizes)
    return c, PR.scores_ref(c['s'], c['t'])


def _f32_scores(r, sigmoid):
    """What a device would report, up to rounding: the float64 score in float32."""
    return (r['p'] if sigmoid else r['raw']).to(F32)


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize('H', HS)
def test_select_ref_is_pinned_to_the_count_references(H):
    c, r = _case(H)
    gp, N = c['graph_ptr'], c['N']
    ei = PR.edges_case(c, 2, 3)
    for sigmoid, thr in SR.CASES:
        sc = _f32_scores(r, sigmoid)
        for g in (gp, None):
            for skip in (False, True):
                row_ptr, col = SR.select_ref(sc, g, thr, skip)
                n = row_ptr[1:] - row_ptr[:-1]
                assert int(row_ptr[0]) == 0 and torch.equal(n, PR.row_counts(sc, g, thr, skip))
                rows = torch.repeat_interleave(torch.arange(N), n)
                mask = PR.candidate_mask(N, g, skip)
                assert bool(mask[rows, col].all()) and bool((sc[rows, col] > thr).all())
                assert int(((sc > thr) & mask).sum()) == col.numel()                    # nothing above the threshold is left out
                same = rows[1:] == rows[:-1]
                assert bool((col[1:] > col[:-1])[same].all())                           # ascending inside a row
                # by target: the same pairs, listed the other way round
                tp, tc = SR.select_ref(sc, g, thr, skip, by='dst')
                assert tc.numel() == col.numel() and torch.equal(SR.selected_matrix(tp, tc, N), SR.selected_matrix(row_ptr, col, N).T)
        # per graph: the predicted positives of graph_counts are the lists' lengths summed over the graph's rows
        row_ptr, _ = SR.select_ref(sc, gp, thr, False)
        gpt = torch.tensor(gp)
        assert torch.equal(row_ptr[gpt[1:]] - row_ptr[gpt[:-1]], PR.graph_counts(sc, ei, gp, thr)[:, 1])
    with pytest.raises(ValueError):
        SR.select_ref(sc, gp, 0.5, False, by='both')


def test_select_ref_never_selects_a_nan_and_is_strict():
    sc = torch.tensor([[0.5, 0.7, float('nan')], [float('nan'), 0.5000001, 0.2], [0.9, 0.5, 0.6]], dtype=F32)
    row_ptr, col = SR.select_ref(sc, None, 0.5)
    assert row_ptr.tolist() == [0, 1, 2, 4] and col.tolist() == [1, 1, 0, 2]
    row_ptr, col = SR.select_ref(sc, [0, 2, 3], 0.5, skip_self=True)
    assert row_ptr.tolist() == [0, 1, 1, 1] and col.tolist() == [1]
    row_ptr, col = SR.select_ref(sc, None, 0.5, by='dst')
    assert row_ptr.tolist() == [0, 1, 3, 4] and col.tolist() == [2, 0, 1, 2]


# ------------------------------------------------------------------------------------------------ the builders
@pytest.mark.parametrize('H', HS)
def test_builder_properties(H):
    """What the device tests rely on: graph borders inside tiles, a row whose selection spans >= 3 column tiles, a row (with candidates)
    that selects nothing and one that selects every candidate, at every threshold of CASES; the planted rows of topk_case still there."""
    c, r = _case(H)
    gp, N, info = c['graph_ptr'], c['N'], c['info']
    assert [b - a for a, b in zip(gp, gp[1:])] == list(PR.TOPK_SIZES) and any(b % 64 for b in gp[1:-1])
    assert info['edge_row'] is not None and info['self_row'] is not None and len(info['ties']) == 3
    full, empty = info['full_row'], info['empty_row']
    for sigmoid, thr in SR.CASES:
        ref, bound = SR.reported(r, sigmoid)
        for shift in (-1, 1):                               # beyond doubt: the same at threshold -/+ bound
            row_ptr, col = SR.select_ref(ref + shift * bound, gp, thr)
            n = row_ptr[1:] - row_ptr[:-1]
            ncand = PR.candidate_mask(N, gp, False).sum(1)
            assert int(n[full]) == int(ncand[full]) == 2 and int(n[empty]) == 0 and int(ncand[empty]) == 2
            spans = [len({int(v) // 64 for v in col[int(row_ptr[u]):int(row_ptr[u + 1])]}) for u in range(gp[-2], N)]
            assert max(spans) >= 3
            assert int(n.max()) > 64                        # a list longer than one tile: the cursor crosses tile borders
        u, v0, v1, vx = info['edge_row']
        assert bool(ref[u, vx] - bound[u, vx] > thr)        # the next graph's first node is above the threshold and must stay out
        us = info['self_row']
        assert bool(ref[us, us] - bound[us, us] > thr)      # self is above the threshold: skip_self has something to skip


def test_empty_middle_builder():
    c, r = _case(32, 1, SR.EMPTY_MIDDLE_SIZES)
    gp = c['graph_ptr']
    assert gp == [0, 5, 5, 75, 77, 77, 143] and c['info']['full_row'] == 75 and c['info']['empty_row'] == 76
    row_ptr, col = SR.select_ref(r['p'].to(F32), gp, 0.5)
    n = row_ptr[1:] - row_ptr[:-1]
    assert int(n[75]) == 2 and int(n[76]) == 0 and int(n.sum()) > 0


@pytest.mark.parametrize('H', HS)
def test_band_around_the_thresholds_is_narrow(H):
    """The share of candidate pairs within their bound of the threshold, from float64 alone, for every case the device test of the
    float64 check uses: at most 1e-3 (measured: at most 1.2e-4 for topk_case at these seeds)."""
    worst = 0.0
    for seed in (1, 2, 3):
        c, r = _case(H, seed)
        for g in (c['graph_ptr'], None):
            mask = PR.candidate_mask(c['N'], g, False)
            for sigmoid, thr in SR.CASES:
                ref, bound = SR.reported(r, sigmoid)
                worst = max(worst, PR.band_fraction(ref, bound, thr, mask))
    print('SEL band H=%d | worst share of candidates within their bound of a threshold %.3g' % (H, worst))
    assert worst <= 1e-3


# ------------------------------------------------------------------------------------------------ planted defects
@functools.lru_cache(maxsize=None)
def _defect_scores():
    """float32 scores of the H = 32 case with what the defects need: entries EQUAL to the threshold and NaNs inside long rows."""
    c, r = _case(32)
    sc = r['p'].to(F32).clone()
    gp = c['graph_ptr']
    u = gp[-2] + 7
    sc[u, gp[-2] + 3] = 0.5
    sc[u, gp[-2] + 150] = 0.5
    sc[u + 1, gp[-2] + 90] = float('nan')
    sc[gp[5] + 1, gp[5] + 70] = float('nan')
    return c, sc


def test_the_restated_fill_without_a_defect_passes_both_checkers():
    c, sc = _defect_scores()
    _, r = _case(32)
    for g, skip in ((c['graph_ptr'], False), (None, True)):
        row_ptr, col, score = SR.restated_fill(sc, g, 0.5, skip)
        assert SR.check_select(row_ptr, col, score, sc, g, 0.5, skip) == []
        assert SR.UNWRITTEN not in col.tolist()
    # and the float64 check on unmodified scores
    clean = r['p'].to(F32)
    row_ptr, col, _ = SR.restated_fill(clean, c['graph_ptr'], 0.5, True)
    assert SR.check_band(row_ptr, col, r['p'], r['dq'], c['graph_ptr'], 0.5, True) == []


@pytest.mark.parametrize('defect', SR.DEFECTS)
def test_planted_defects_are_caught_by_the_exact_checker(defect):
    """cursor reset at a tile border, descending order inside a block, the next graph's first node admitted, self not skipped, >= for >,
    a NaN selected: each makes check_select (the check of the device file) report."""
    c, sc = _defect_scores()
    gp = c['graph_ptr']
    row_ptr, col, score = SR.restated_fill(sc, gp, 0.5, True, defect=defect)
    bad = SR.check_select(row_ptr, col, score, sc, gp, 0.5, True)
    print('SEL defect %s | %s' % (defect, bad))
    assert bad


@pytest.mark.parametrize('defect', ('cursor_reset', 'descending_block', 'next_graph', 'self'))
def test_planted_defects_are_caught_by_the_float64_checker(defect):
    """The defects that do not sit on the threshold itself are also outside the float64 bounds."""
    c, r = _case(32)
    gp = c['graph_ptr']
    row_ptr, col, _ = SR.restated_fill(r['p'].to(F32), gp, 0.5, True, defect=defect)
    assert SR.check_band(row_ptr, col, r['p'], r['dq'], gp, 0.5, True)


def test_a_wrong_score_or_a_transposed_list_is_caught():
    c, sc = _defect_scores()
    gp = c['graph_ptr']
    row_ptr, col, score = SR.restated_fill(sc, gp, 0.5, False)
    wrong = score.clone()
    wrong[5] = torch.nextafter(wrong[5], torch.tensor(2.0))
    assert SR.check_select(row_ptr, col, wrong, sc, gp, 0.5, False)
    assert SR.check_select(row_ptr, col, score, sc, gp, 0.5, False, by='dst')           # lists by source are not lists by target
    tp, tc, ts = SR.restated_fill(sc.T.contiguous(), gp, 0.5, False)
    assert SR.check_select(tp, tc, ts, sc, gp, 0.5, False, by='dst') == []


# ------------------------------------------------------------------------------------------------ host-only paths
def test_host_refusals_need_no_gpu():
    from deepgate import _hip, ops, pairs
    s = torch.zeros(4, 16)
    with pytest.raises(_hip.HipLibraryError, match="by must be 'src'"):
        ops.pair_select(s, s, by='both')
    with pytest.raises(_hip.HipLibraryError, match='MGV_EUNSUPPORTED'):
        ops.pair_select(torch.zeros(4, 48), torch.zeros(4, 48))
    with pytest.raises(_hip.HipLibraryError, match='GPU'):
        ops.pair_select(s, s)                               # no CPU implementation behind it
    with pytest.raises(_hip.HipLibraryError) as e:
        pairs._select_room(98113, False, 50000, None)
    msg = str(e.value)
    assert '98113' in msg and '50000' in msg and 'threshold' in msg and 'pair_topk' in msg
    with pytest.raises(_hip.HipLibraryError) as e:
        pairs._select_room(3 * 2 ** 30, True, None, 2 ** 30)
    msg = str(e.value)
    assert str(3 * 2 ** 30) in msg and '24.0 GiB' in msg and 'pair_topk' in msg
    pairs._select_room(10, True, 10, 80)                    # exactly at both limits: accepted
    pairs._select_room(0, False, 0, 0)


def test_the_header_declares_both_entries_with_their_reference_lines():
    from deepgate import _hip
    sigs = _hip.parse_header()
    assert len(sigs['mgv_pair_select_count']) == 13 and len(sigs['mgv_pair_select_fill']) == 16
    with open(_hip.HEADER_PATH) as f:
        text = f.read()
    for name in ('mgv_pair_select_count', 'mgv_pair_select_fill'):
        head = text[:text.index('int %s(' % name)]
        comment = head[head.rindex('/*'):]
        assert 'digae_layer.py:31-33' in comment and 'digae_model.py:118-122' in comment
