"""Pins tests/concord_ref.py, the restatement of mgv_concord_counts (csrc/concordance.hip), on the CPU: its plain loops equal its
vectorised form on seeded cases and reproduce what the reference's get_function_acc returned when it was made to visit every comparison
(tests/golden/g10_function_acc.npz); closed forms; each planted defect changes a count on a designed case; the segment table of
ops.pair_segments against its numpy twin; the header's declaration; the host refusals of the entry through ctypes (nothing is
launched, no pointer is followed: no GPU needed); the --val_func_acc flag."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import concord_ref as CR  # noqa: E402
from conftest import PKG_PARENT, load_golden  # noqa: E402

F32 = np.float32
T = CR.TILE


def _ops():
    if PKG_PARENT not in sys.path:
        sys.path.insert(0, PKG_PARENT)
    from deepgate import ops
    return ops


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('P, seg', [(0, None), (1, None), (2, None), (37, None), (90, [0, 0, 1, 40, 40, 42, 90]), (60, [0, 25, 80]),
                                    (50, [5, 30, 45])])
@pytest.mark.parametrize('nan_share', [0.0, 0.1])
def test_the_loops_equal_the_vectorised_form(P, seg, nan_share):
    gt, pred = CR.random_case(P, 7 * P + int(10 * nan_share), nan_share=nan_share)
    gaps = (0.0, 0.05, 0.1, 0.15, 5.0)
    with np.errstate(invalid='ignore'):
        a = CR.counts_loops(gt, pred, seg, gaps)
    b = CR.counts_numpy(gt, pred, seg, gaps)
    assert a.shape == (max(len(seg) - 1, 1) if seg is not None else 1, 5, 3)
    assert np.array_equal(a, b)
    assert (a[:, 4] == 0).all()                                   # a gap no comparison reaches
    assert (a[:, :, 1] + a[:, :, 2] <= a[:, :, 0]).all()
    if P > 2 and nan_share == 0.0:
        assert a[:, 0, 0].sum() > 0 and a[:, 0, 2].sum() > 0      # the cases are not empty: eligible comparisons, prediction ties


def test_the_restatement_reproduces_the_reference_on_the_fixture():
    """acc of the fixture is the return value of the reference's get_function_acc after it visited every comparison once."""
    z = load_golden('g10_function_acc')
    hf, pairs, tt = torch.from_numpy(z['hf']), z['pairs'], z['tt_dis']
    assert tt.dtype == F32 and hf.dtype == torch.float32
    pred = (1 - torch.cosine_similarity(hf[pairs[0]], hf[pairs[1]], eps=1e-8)).numpy()
    assert pred.dtype == F32
    counts = CR.counts_loops(tt, pred, z['seg_ptr'], (CR.MIN_GAP,))
    assert np.array_equal(counts, CR.counts_numpy(tt, pred, z['seg_ptr'], (CR.MIN_GAP,)))
    acc = CR.accuracy(counts)[:, 0]
    assert np.array_equal(acc, z['acc']), (acc, z['acc'])
    assert (np.diff(z['seg_ptr']) <= 12).all()                    # at most 66 comparisons: the function's stop at 100 is never reached
    assert z['acc'][6] == -1 and counts[6, 0, 0] == 0             # nothing eligible
    assert counts[4, 0, 2] >= 2                                   # the planted prediction ties are eligible ties
    # circuit 5: 0 beside float32(0.05) is eligible (>=), beside the float one ulp below it is not, the equal pair is not
    lo = int(z['seg_ptr'][5])
    g5 = tt[lo:lo + 5]
    assert g5[1] - g5[0] == F32(0.05) and 0 < g5[2] - g5[0] < F32(0.05) and g5[3] == g5[4]
    sub = lambda i, j: CR.counts_loops(g5[[i, j]], [0.0, 1.0], None, (CR.MIN_GAP,))[0, 0, 0]       # noqa: E731
    assert (sub(0, 1), sub(0, 2), sub(3, 4)) == (1, 0, 0)
    segs, ok = CR.segments_numpy(pairs[0], pairs[1], z['graph_ptr'])
    assert ok and np.array_equal(segs, z['seg_ptr'])


@pytest.mark.parametrize('P', [1, 2, 3, T - 1, T + 1])
@pytest.mark.parametrize('k', [1, 2, 5])
def test_closed_forms_on_the_ladder(P, k):
    gt = CR.ladder(P)
    gap = (k * 2.0 ** -17,)
    want = CR.closed_form(P, k)
    fn = CR.counts_loops if P <= 3 else CR.counts_numpy
    assert fn(gt, gt, None, gap)[0, 0].tolist() == [want, want, 0]
    assert fn(gt, -gt, None, gap)[0, 0].tolist() == [want, 0, 0]
    assert CR.closed_form(70001, 1) > 2 ** 31                     # the size the device test takes past 32 bits


LADDER = CR.ladder(T + 1)
DEFECT_CASES = {
    # defect: (gt, pred, seg_ptr, gaps)
    'gt_for_ge': (np.array([0.0, F32(0.05)], dtype=F32), [0.0, 1.0], None, (0.05,)),
    'no_nonzero': ([0.3, 0.3], [0.0, 1.0], None, (0.0,)),
    'tie_correct': ([0.0, 1.0], [0.5, 0.5], None, (0.05,)),
    'diagonal+no_nonzero': ([0.0, 1.0], [0.0, 1.0], None, (0.0,)),
    'both': ([0.0, 1.0], [0.0, 1.0], None, (0.05,)),
    'cross': ([0.0, 1.0], [0.0, 1.0], [0, 1, 2], (0.05,)),
    'last_row': (LADDER, LADDER, None, (2.0 ** -17,)),
    'last_col': (LADDER, LADDER, None, (2.0 ** -17,)),
}


@pytest.mark.parametrize('defect', sorted(DEFECT_CASES))
def test_each_planted_defect_changes_a_count_on_its_designed_case(defect):
    gt, pred, seg, gaps = DEFECT_CASES[defect]
    good = CR.counts_loops(gt, pred, seg, gaps)
    bad = CR.counts_loops(gt, pred, seg, gaps, defect=defect)
    assert np.array_equal(good, CR.counts_numpy(gt, pred, seg, gaps))
    assert not np.array_equal(good, bad), defect


def test_the_diagonal_alone_can_never_show():
    """dd = gt[p] - gt[p] is 0, or NaN where gt[p] is NaN or infinite: never eligible.  Including p == q is therefore no defect a count
    could reveal by itself (it shows with the dd != 0 test gone, above); recorded here so that nobody looks for a case."""
    gt = np.array([0.0, 1.0, np.nan, np.inf, -np.inf, 1e-45, 3.0], dtype=F32)
    pred = np.array([0.0, np.nan, 1.0, 2.0, 2.0, 5.0, np.inf], dtype=F32)
    with np.errstate(invalid='ignore'):
        assert np.array_equal(CR.counts_loops(gt, pred, None, (0.0, 0.05)), CR.counts_loops(gt, pred, None, (0.0, 0.05), defect='diagonal'))


# ------------------------------------------------------------------------------------------------ segments
def test_the_segment_table_and_its_refusals():
    ops = _ops()
    gp = [0, 10, 10, 25, 40]
    first = np.array([1, 3, 9, 12, 24, 24, 30], dtype=np.int64)
    second = np.array([2, 0, 9, 20, 10, 11, 39], dtype=np.int64)
    seg, ok = CR.segments_numpy(first, second, gp)
    assert ok and seg.tolist() == [0, 3, 3, 6, 7]
    tseg, tok = ops.segment_table(torch.from_numpy(first), gp, torch.from_numpy(second))
    assert bool(tok) and tseg.tolist() == seg.tolist()
    assert ops.pair_segments(torch.from_numpy(np.stack([first, second])), gp).tolist() == seg.tolist()
    assert ops.pair_segments(torch.from_numpy(np.stack([first, second])), gp).dtype == torch.int32
    bad = {'crosses circuits': (first, np.array([2, 0, 10, 20, 10, 11, 39])), 'ungrouped': (first[[0, 3, 1, 2, 4, 5, 6]], second[[0, 3, 1, 2, 4, 5, 6]]),
           'outside the batch': (np.array([1, 40]), np.array([2, 39])), 'negative': (np.array([1, 3]), np.array([-1, 2]))}
    for why, (a, b) in bad.items():
        assert not CR.segments_numpy(a, b, gp)[1], why
        assert not bool(ops.segment_table(torch.as_tensor(a), gp, torch.as_tensor(b))[1]), why
        with pytest.raises(ValueError):
            ops.pair_segments(torch.as_tensor(np.stack([a, b])), gp)
    # no pairs at all, and a batch whose last circuits list nothing
    e = np.zeros(0, dtype=np.int64)
    assert CR.segments_numpy(e, e, gp)[0].tolist() == [0, 0, 0, 0, 0] and CR.segments_numpy(e, e, gp)[1]
    assert ops.pair_segments(torch.zeros((2, 0), dtype=torch.int64), gp).tolist() == [0, 0, 0, 0, 0]
    assert ops.pair_segments(torch.tensor([[1], [2]]), gp).tolist() == [0, 1, 1, 1, 1]

    class Box:
        pass
    box = Box()
    pi = torch.from_numpy(np.stack([first, second]))
    assert ops.pair_segments(pi, gp, cache=box) is ops.pair_segments(pi, gp, cache=box)        # built once per batch


def test_the_tile_edge_is_stated_once_per_side():
    ops = _ops()
    with open(os.path.join(PKG_PARENT, 'csrc', 'concordance.hip')) as f:
        src = f.read()
    assert int(re.search(r'constexpr int kConcordTile = (\d+);', src).group(1)) == ops.CONCORD_TILE == CR.TILE
    assert int(re.search(r'constexpr int kConcordMaxGaps = (\d+);', src).group(1)) == ops.CONCORD_MAX_GAPS == 8
    assert ops.MIN_GAP == CR.MIN_GAP == 0.05


# ------------------------------------------------------------------------------------------------ the header and the host refusals
def test_the_header_declares_the_entry_with_its_reference_lines():
    from deepgate import _hip
    sigs = _hip.parse_header()
    assert len(sigs['mgv_concord_counts']) == 9
    with open(_hip.HEADER_PATH) as f:
        text = f.read()
    head = text[:text.index('int mgv_concord_counts(')]
    comment = re.sub(r'\s+', ' ', head[head.rindex('/* ----'):].replace('\n *', ' '))
    assert 'utils/utils.py:111-147' in comment and 'trainer.py:158-160' in comment
    for words in ('dd != 0 && fabsf(dd) >= gaps[j]', '(dd > 0 && de > 0) || (dd < 0 && de < 0)', 'de == 0', 'A NaN in gt', 'a NaN in pred',
                  'never cross segments', 'p == q is never counted', 'clamped into [0, P)', 'HOST memory', 'never synchronises', 'OVERWRITTEN',
                  'P < 0 or P > 2^31 - 1', 'G < 0', 'B outside [1, 8]', 'a NULL out', 'a NULL gt, pred or gaps_host with P > 0',
                  'a NaN or negative gap', 'MGV_EINVAL', 'P = 0 zeroes out and launches nothing', 'no floating-point atomics'):
        assert words in comment, words


def _entry(P=4, gaps=(0.05,), B=None, G=0, out=4096, gt=1024, pred=2048, gaps_null=False):
    """The entry with dummy device pointers (never followed: every call here is refused before anything is launched or zeroed)."""
    from deepgate import _hip
    lib = _hip.load()
    arr = (ctypes.c_float * max(len(gaps), 1))(*gaps)
    return lib.mgv_concord_counts(P, ctypes.c_void_p(gt), ctypes.c_void_p(pred), None, G, None if gaps_null else arr,
                                  len(gaps) if B is None else B, ctypes.c_void_p(out), None)


@pytest.mark.parametrize('why, kw', [
    ('B = 0', dict(B=0)), ('B = 9', dict(gaps=(0.1,) * 9)), ('a NaN gap', dict(gaps=(0.05, float('nan')))),
    ('a negative gap', dict(gaps=(-0.01,))), ('P < 0', dict(P=-1)), ('P > 2^31 - 1', dict(P=2 ** 31)), ('a NULL out', dict(out=None)),
    ('G < 0', dict(G=-1)), ('a NULL gt', dict(gt=None)), ('a NULL pred', dict(pred=None)), ('NULL gaps', dict(gaps_null=True)),
    ('a NULL out at P = 0', dict(P=0, out=None)), ('a NaN gap at P = 0', dict(P=0, gaps=(float('nan'),)))])
def test_the_host_refusals_return_einval(why, kw):
    assert _entry(**kw) == -1, why


def test_ops_refuses_bad_gaps_on_the_host():
    _ops()
    from deepgate import metrics
    for gaps in ((), (0.1,) * 9, (float('nan'),), (0.05, -1.0)):
        with pytest.raises(ValueError):
            metrics._concord_gaps(gaps)
    g = metrics._concord_gaps([0.05, 0.1])
    assert list(g) == [float(F32(0.05)), float(F32(0.1))]        # float32 once, on the host


def test_val_func_acc_flag_defaults_off():
    if PKG_PARENT not in sys.path:
        sys.path.insert(0, PKG_PARENT)
    from config import get_parse_args
    assert get_parse_args(['--type', 'aig']).val_func_acc is False
    assert get_parse_args(['--type', 'aig', '--val_func_acc']).val_func_acc is True
    assert get_parse_args(['--type', 'aig', '--val_func_acc']).val_auc is False
