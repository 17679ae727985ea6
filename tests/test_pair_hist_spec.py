"""Pins tests/pair_hist_ref.py on the CPU: the restated walk equals the brute-force bins, counts_above of it equals the count entries'
references at every edge (PR.row_counts / ER.upper_select_ref), every planted defect changes the result, and the bracket logic of
ops.sim_threshold_for (ops.threshold_search, driven here by a CPU stand-in for the profile walk) keeps its guarantees.

The matrices are float32 stand-ins of what a device reports: ER.chain_f32 of ER.unit_f32 rows for the cosine, the float32 rounding of
PR.scores_ref for the decoder.  The NaN defect is shown on ER.nan_case: sim_case and select_case hold no NaN."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import embed_sim_ref as ER  # noqa: E402
import pair_hist_ref as HR  # noqa: E402
import pair_scores_ref as PR  # noqa: E402
import pair_select_ref as SR  # noqa: E402
from conftest import PKG_PARENT  # noqa: E402

F64, F32, I64 = torch.float64, torch.float32, torch.int64
H = 16
TABLES = ('A', 'B', 'D', 'one', 'wide')


@functools.lru_cache(maxsize=None)
def _cos(kind='sim'):
    c = ER.CASES[kind](H, 1) if kind in ER.CASES else HR.many_graphs_case(H, 1)
    return c, ER.chain_f32(ER.unit_f32(c['x'])[0])


@functools.lru_cache(maxsize=None)
def _dec(sigmoid, kind='select'):
    c = SR.select_case(H, 1) if kind == 'select' else HR.many_graphs_case(H, 1)
    r = PR.scores_ref(c['s'], c['t'])
    return c, (r['p'] if sigmoid else r['raw']).to(F32)


def test_the_tables_are_what_the_device_tests_use():
    for name in TABLES:
        e = HR.edges_f32(name)
        assert e.dtype == F32 and bool((e[1:] > e[:-1]).all())
    assert HR.edges_f32('A').numel() == 64 and HR.edges_f32('B').numel() == 20 and HR.edges_f32('wide').numel() == HR.MAX_EDGES
    assert HR.EDGES['D'] == (-2.0, 0.0, 1.5) and HR.EDGES['one'] == (0.999,)
    assert float(HR.edges_f32('A')[0]) == -1 + 0.5 / 32 and float(HR.edges_f32('B')[0]) == 0.5
    assert float(HR.edges_f32('B')[-1]) == float(torch.tensor(1 - 2.0 ** -20, dtype=F32)) < 1.0


@pytest.mark.parametrize('kind', ['sim', 'empty_middle', 'nan', 'many'])
def test_the_symmetric_restatement_equals_the_brute_force_bins(kind):
    c, cos = _cos(kind)
    gp, N = c['graph_ptr'], c['N']
    cands = int((ER.upper_mask(N, gp) & ~torch.isnan(cos)).sum())
    for name in TABLES:
        want = HR.brute_hist(cos, gp, name, True)
        got = HR.restated_hist(cos, gp, name, True)
        assert torch.equal(got, want), (kind, name)
        assert int(want.sum()) == cands
        assert torch.equal(HR.counts_above(want), HR.select_totals(cos, gp, name, True)), (kind, name)
    d = HR.brute_hist(cos, gp, 'D', True)
    assert int(d[:, 0].sum()) == 0 and int(d[:, 3].sum()) == 0          # nothing at or below -2, nothing above 1.5
    if kind == 'sim':
        zeros = c['info']['zeros']
        assert int(d[:, 1].sum()) >= 64 and all(float(cos[z].abs().max()) == 0 for z in zeros)     # cosines of exactly 0 lie in bin 1
    if kind == 'many':
        assert len(gp) - 1 == 64 and N <= 3 * 64 and max(c['sizes']) == 3 and min(c['sizes']) == 1


@pytest.mark.parametrize('sigmoid,skip', [(True, False), (False, False), (False, True)])
def test_the_general_restatement_equals_the_brute_force_bins(sigmoid, skip):
    for kind in ('select', 'many'):
        c, sc = _dec(sigmoid, kind)
        gp, N = c['graph_ptr'], c['N']
        for g in (gp, None):
            for name in ('A', 'D', 'wide'):
                want = HR.brute_hist(sc, g, name, False, skip)
                assert torch.equal(HR.restated_hist(sc, g, name, False, skip_self=skip), want), (kind, name, g is None)
                assert int(want.sum()) == int(PR.candidate_mask(N, g, skip).sum())
                assert torch.equal(HR.counts_above(want), HR.select_totals(sc, g, name, False, skip)), (kind, name)


@pytest.mark.parametrize('defect', HR.DEFECTS)
def test_every_planted_defect_changes_the_result(defect):
    """On sim_case (both forms: its cosines hold exact zeros for `>=`) and select_case; the NaN defect on nan_case."""
    kind = 'nan' if defect == 'nan' else 'sim'
    c, cos = _cos(kind)
    gp = c['graph_ptr']
    changed = []
    for name in ('A', 'D'):
        good = HR.restated_hist(cos, gp, name, True)
        changed.append(not torch.equal(HR.restated_hist(cos, gp, name, True, defect=defect), good))
    if defect == 'last_bin':                                # the last bin of D is empty by design: the defect shows on A alone
        assert changed[0]
    elif defect == 'ge':                                    # a score must EQUAL an edge: the zero rows' cosines and the 0.0 of D
        assert changed[1]
    else:
        assert all(changed), (defect, changed)
    if defect in HR.SYM_ONLY:
        return
    # the general form: the cosine matrix without self, and the decoder's case
    good = HR.restated_hist(cos, gp, 'D', False, skip_self=True)
    assert not torch.equal(HR.restated_hist(cos, gp, 'D', False, defect=defect, skip_self=True), good) or defect == 'last_bin'
    if defect not in ('nan', 'ge'):                         # select_case has neither a NaN nor a score that equals an edge
        c2, sc = _dec(False)
        good = HR.restated_hist(sc, c2['graph_ptr'], 'A', False)
        assert not torch.equal(HR.restated_hist(sc, c2['graph_ptr'], 'A', False, defect=defect), good)


# ------------------------------------------------------------------------------------------------ the bracket logic
def _ops():
    if PKG_PARENT not in sys.path:
        sys.path.insert(0, PKG_PARENT)
    from deepgate import ops
    return ops


def _walk(cos, gp, calls):
    def profile(e):
        calls.append(e.clone())
        assert e.dtype == F32 and e.dim() == 1 and 1 <= e.numel() <= 64 and bool((e[1:] > e[:-1]).all())
        return HR.brute_hist(cos, gp, e.tolist(), True)
    return profile


def _count(cos, gp, thr):
    return int(((cos > thr) & ER.upper_mask(cos.shape[0], gp)).sum())


@pytest.mark.parametrize('max_pairs', [0, 1, 3, 100, 'all'])
def test_the_threshold_search_keeps_its_guarantees(max_pairs):
    ops = _ops()
    c, cos = _cos('sim')
    gp, N = c['graph_ptr'], c['N']
    allp = int(ER.upper_mask(N, gp).sum())
    P = allp if max_pairs == 'all' else max_pairs
    for lo in (0.0, -2.0):
        calls = []
        r = ops.threshold_search(_walk(cos, gp, calls), P, lo=lo, hi=2.0, bins=64, max_rounds=6)
        thr = r['threshold']
        assert isinstance(thr, float) and float(torch.tensor(thr, dtype=F32)) == thr and len(calls) <= 6
        assert r['pairs'] <= P and r['pairs'] == _count(cos, gp, thr)
        assert r['tight'] is True
        for e in calls:
            assert float(e[0]) >= lo and float(e[-1]) <= 2.0
        if r['lower'] is None:                              # the count at lo already fits
            assert thr == lo and _count(cos, gp, lo) <= P and len(calls) == 1 and r['pairs_lower'] is None
        else:
            assert r['lower'] < thr and r['pairs_lower'] > P and r['pairs_lower'] == _count(cos, gp, r['lower'])
            nxt = float(torch.nextafter(torch.tensor(r['lower'], dtype=F32), torch.tensor(INF32)))
            assert nxt == thr                               # tight: no float32 strictly between the two ends
    assert ops.threshold_search(_walk(cos, gp, []), allp, lo=-2.0)['lower'] is None
    assert ops.threshold_search(_walk(cos, gp, []), _count(cos, gp, 0.0), lo=0.0)['threshold'] == 0.0


INF32 = float('inf')


def test_the_threshold_search_stops_after_max_rounds_and_refuses_a_bad_bracket():
    ops = _ops()
    c, cos = _cos('sim')
    gp = c['graph_ptr']
    calls = []
    r = ops.threshold_search(_walk(cos, gp, calls), 3, lo=-2.0, bins=4, max_rounds=2)
    assert len(calls) == 2 and r['tight'] is False and r['lower'] < r['threshold']
    assert r['pairs'] <= 3 < r['pairs_lower'] and r['pairs'] == _count(cos, gp, r['threshold'])
    with pytest.raises(Exception):
        ops.threshold_search(_walk(cos, gp, []), -1)
    with pytest.raises(Exception):
        ops.threshold_search(_walk(cos, gp, []), 3, lo=2.0)
    # an upper end above which pairs remain cannot be a bracket
    with pytest.raises(Exception, match='upper end'):
        ops.threshold_search(_walk(cos, gp, []), 0, lo=-2.0, hi=0.0)
    e = ops.counts_above(torch.tensor([[5, 1, 0, 2], [0, 0, 7, 0]]))
    assert e.tolist() == [[3, 2, 2], [7, 7, 0]]
