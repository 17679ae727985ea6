"""CPU pins of tests/pair_scores_ref.py, the float64 restatement behind tests/test_hip_pair_scores.py: it reproduces the reference's own
recorded forward_all (fixture dec_all of g3_ops), float64 autograd and torch.topk; its case builders have the properties the device
tests rely on; and the defects those tests are there to catch land at least 10 x outside the device bounds, or change an integer."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_scores_ref as PR  # noqa: E402
from conftest import load_golden  # noqa: E402

F64, F32 = torch.float64, torch.float32


def _fixture():
    z = load_golden('g3_ops')
    return torch.from_numpy(z['dec_s']), torch.from_numpy(z['dec_t']), torch.from_numpy(z['dec_all'])


def test_restatement_equals_the_recorded_forward_all():
    s, t, ref = _fixture()
    assert ref.shape == (30, 30)
    r = PR.scores_ref(s, t)
    err = float((r['p'] - ref.to(F64)).abs().max())
    print('dec_all: float64 restatement against the recorded float32 output: %.2g' % err)
    assert err <= 2e-6


@pytest.mark.parametrize('sigmoid', [True, False])
def test_gradients_equal_float64_autograd(sigmoid):
    c = PR.dense_case(37, 70, 32, 3, sigmoid)
    s, t = c['s'].to(F64).requires_grad_(True), c['t'].to(F64).requires_grad_(True)
    out = s @ t.T
    out = torch.sigmoid(out) if sigmoid else out
    out.backward(c['g'].to(F64))
    r = PR.grads_ref(c['s'], c['t'], c['g'], sigmoid)
    for k, ref in (('ds', s.grad), ('dt', t.grad)):
        assert float((r[k] - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max())), k
        assert bool((r[k + '_bound'] > 0).all())


def test_topk_equals_torch_topk_on_a_tie_free_case():
    c = PR.topk_case(16, 5, plant=False)
    raw = PR.scores_ref(c['s'], c['t'])['raw']
    idx, score = PR.topk_ref(raw, None, 8, False, sigmoid=True)
    tv, ti = torch.topk(raw, 8, dim=1)
    assert torch.equal(idx.long(), ti)
    assert float((score - torch.sigmoid(tv)).abs().max()) <= 1e-15     # (scalar and vectorised float64 sigmoid: the last bit)
    assert torch.equal(PR.row_counts(torch.sigmoid(raw), None, 0.5), (raw > 0).sum(1))


def test_chain_length_is_the_padded_walk():
    assert [PR.chain_length(n) for n in (0, 1, 64, 65, 257)] == [0, 64, 64, 128, 320]


# ------------------------------------------------------------------------------------------------ builders
@pytest.mark.parametrize('H', [16, 32, 64, 128])
def test_topk_case_properties(H):
    c = PR.topk_case(H, 1)
    gp, info = c['graph_ptr'], c['info']
    assert gp[-1] == c['N'] == sum(PR.TOPK_SIZES)
    inner = gp[1:-1]
    assert any(b % PR.TILE for b in inner)                                   # graph boundaries inside row and column tiles
    assert any(gp[i] // PR.TILE != (gp[i + 1] - 1) // PR.TILE for i in range(len(gp) - 1) if gp[i + 1] > gp[i])   # a graph over several tiles
    assert any(gp[i] // PR.TILE == (gp[i + 1]) // PR.TILE for i in range(len(gp) - 1))                            # several graphs in one tile
    a, b, d = info['ties']
    assert torch.equal(c['t'][a], c['t'][b]) and torch.equal(c['t'][a], c['t'][d])
    assert a // PR.TILE != b // PR.TILE                                     # exact ties across a column-tile boundary ...
    g_of = lambda v: max(i for i in range(len(gp) - 1) if gp[i] <= v)       # noqa: E731
    assert g_of(a) == g_of(b) == g_of(d)                                    # ... inside one graph
    r = PR.scores_ref(c['s'], c['t'])
    lo, hi = gp[g_of(a)], gp[g_of(a) + 1]
    first = PR.topk_ref(r['raw'], gp, 4, False)[0][lo:hi]
    tied = (first[:, 0] == a) & (first[:, 1] == b) & (first[:, 2] == d)
    assert int(tied.sum()) >= 8                                             # the tie decides the head of several rows' lists
    u, v0, v1, vx = info['edge_row']
    order = torch.argsort(r['raw'][u], descending=True)[:3].tolist()
    assert order == [vx, v1, v0] and g_of(vx) == g_of(u) + 1 and g_of(v0) == g_of(v1) == g_of(u)
    us = info['self_row']
    assert int(torch.argmax(r['raw'][us])) == us
    # near-threshold condition: at most 1e-3 of the pairs within their bound of the threshold
    mask = PR.candidate_mask(c['N'], gp, False)
    assert PR.band_fraction(r['p'], r['dq'], 0.5, mask) <= 1e-3
    assert PR.band_fraction(r['raw'], r['raw_bound'], 0.0, mask) <= 1e-3


def test_dense_case_properties():
    for sig in (True, False):
        c = PR.dense_case(257, 129, 64, 2, sig)
        mag = c['s'].abs().max(1).values
        assert float(mag.max() / mag.min()) > (10 if sig else 1000)          # rows carry their own powers of ten
        r = PR.scores_ref(c['s'], c['t'])
        assert PR.band_fraction(r['p'], r['dq'], 0.5, torch.ones_like(r['p'], dtype=torch.bool)) <= 1e-3
    assert PR.dense_case(5, 7, 16, 1)['s'].equal(PR.dense_case(5, 7, 16, 1)['s'])     # seeded


# ------------------------------------------------------------------------------------------------ planted defects
def _worst(val, ref, bound):
    return float(((val - ref).abs() / bound.clamp(min=1e-300)).max())


def test_dense_defects_are_far_outside_the_bounds():
    c = PR.dense_case(65, 130, 32, 4)
    r = PR.scores_ref(c['s'], c['t'])
    stale = torch.full_like(r['p'], float('nan'))           # what a lost tile leaves in the output
    lost_col = r['p'].clone(); lost_col[:, 128:] = stale[:, 128:]             # noqa: E702  a lost last column tile
    lost_row = r['p'].clone(); lost_row[64] = stale[64]                       # noqa: E702  a lost last row of a partial tile
    for bad in (lost_col, lost_row):
        e = (bad - r['p']).abs() / r['dq']
        assert not bool((e <= 1).all())
    # the same with zeros in place of NaN (an output that was cleared first)
    z = r['p'].clone(); z[:, 128:] = 0                                        # noqa: E702
    assert _worst(z, r['p'], r['dq']) >= 10
    z = r['p'].clone(); z[64] = 0                                             # noqa: E702
    assert _worst(z, r['p'], r['dq']) >= 10


def test_backward_defects_are_far_outside_the_bounds():
    c = PR.dense_case(65, 130, 32, 6)
    s, t, g = c['s'].to(F64), c['t'].to(F64), c['g'].to(F64)
    r = PR.grads_ref(c['s'], c['t'], c['g'], True)
    # p (1 - p) forgotten
    assert _worst(g @ t, r['ds'], r['ds_bound']) >= 10
    assert _worst(g.T @ s, r['dt'], r['dt_bound']) >= 10
    # dt built from G instead of G^T (square case, so that the shapes allow it)
    c2 = PR.dense_case(65, 65, 32, 7)
    r2 = PR.grads_ref(c2['s'], c2['t'], c2['g'], True)
    p = PR.scores_ref(c2['s'], c2['t'])['p']
    G = c2['g'].to(F64) * p * (1 - p)
    assert _worst(G @ c2['s'].to(F64), r2['dt'], r2['dt_bound']) >= 10
    # a lost last walked tile
    assert _worst((g * PR.scores_ref(s, t)['p'] * (1 - PR.scores_ref(s, t)['p']))[:, :128] @ t[:128], r['ds'], r['ds_bound']) >= 10


def test_topk_defects_change_the_answer():
    H, k = 32, 4
    c = PR.topk_case(H, 2)
    gp, info, N = c['graph_ptr'], c['info'], c['N']
    r = PR.scores_ref(c['s'], c['t'])
    idx, score = PR.topk_ref(r['raw'], gp, k, True)
    assert PR.check_topk(idx, score, r, gp, k, True, True) == []
    u, v0, v1, vx = info['edge_row']
    # the neighbouring graph's first node visible
    wrong = idx.clone(); wrong[u, 0] = vx                                     # noqa: E702
    assert PR.check_topk(wrong, score, r, gp, k, True, True)
    assert vx not in idx[u].tolist() and idx[u, 0] == v1
    # self not skipped
    us = info['self_row']
    i2, s2 = PR.topk_ref(r['raw'], gp, k, False)
    assert i2[us, 0] == us and us not in idx[us].tolist()
    assert PR.check_topk(i2, s2, r, gp, k, True, True)
    # ties in descending id order: an integer changes (the scores are equal, so only the ids can tell)
    a, b, d = info['ties']
    rows = [x for x in range(N) if idx[x, :3].tolist() == [a, b, d]]
    assert rows
    flipped = idx.clone(); flipped[rows[0], :3] = torch.tensor([d, b, a], dtype=torch.int32)   # noqa: E702
    assert not torch.equal(flipped, idx)
    # the k-th entry dropped
    short = idx.clone(); sh_s = score.clone()                                 # noqa: E702
    full = [x for x in range(N) if idx[x, k - 1] >= 0][0]
    short[full, k - 1] = -1; sh_s[full, k - 1] = -math.inf                    # noqa: E702
    assert PR.check_topk(short, sh_s, r, gp, k, True, True)
    # a lost last column tile of a graph: its best candidates are missing
    cut = r['raw'].clone()
    cut[:, (N - 1) // PR.TILE * PR.TILE:] = float('nan')                       # (a NaN is never selected)
    li, ls = PR.topk_ref(cut, gp, k, True)
    assert PR.check_topk(li, ls, r, gp, k, True, True)


def test_threshold_is_strict():
    """sigma = 0.5 exactly (raw 0) is not a hit: `>=` changes the integer."""
    s = torch.tensor([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    t = torch.tensor([[0.0, 1.0], [1.0, 0.0], [1.0, 1.0]])
    p = PR.scores_ref(s, t)['p']
    strict = PR.row_counts(p, None, 0.5)
    loose = (p >= 0.5).sum(1)
    assert strict.tolist() == [2, 2, 3] and loose.tolist() == [3, 3, 3]
    ei = torch.tensor([[0, 1, 2], [0, 1, 2]])
    assert PR.graph_counts(p, ei, [0, 3], 0.5).tolist() == [[1, 7, 3, 9]]
    assert PR.graph_counts(p, ei, [0, 2, 3], 0.5).tolist() == [[0, 2, 2, 4], [1, 1, 1, 1]]
