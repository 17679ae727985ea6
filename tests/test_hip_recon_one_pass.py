"""The reconstruction loss in one walk of the lists (mgv_recon_step_csr, mgv_recon_step_heavy_lists, mgv_rows_rescale_unless and the
route ops.ReconLossFn takes for a training step), through the C ABI and through ops.

What is asserted, and against what:
  gradient rows   bit-identical to mgv_recon_loss_bwd_csr (+ mgv_recon_heavy_lists) run with a device scalar equal to expect_scale:
                  the walk, its ranges and its arithmetic are the same code;
  counters        equal to mgv_recon_loss_fwd's on the same pairs (the same float dot product, sigmoid and `p > 0.5`);
  sums            against the float64 restatement tests/recon_step_ref.py within the bound derived there (per term, from the
                  reference's data alone), and against mgv_recon_loss_fwd within twice that bound (each is within it of the truth);
  two runs        the same bits (no float atomics anywhere on the route)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import losses_ref as LR  # noqa: E402
import recon_step_ref as SR  # noqa: E402

F64, F32 = torch.float64, torch.float32
U24 = 2.0 ** -24
CASES = [('odd', True, True), ('xcd', True, True), ('one', True, True), ('odd', False, True), ('odd', True, False)]
IDS = ['odd', 'xcd', 'n1', 'Ep0', 'En0']


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _case(H, size, want_pos=True, want_neg=True):
    c = SR.build(H, size, want_pos=want_pos, want_neg=want_neg)
    return c, SR.walk(c['st'], c['pos'], c['neg'])


# ================================================================================================ the builder and the restatement (CPU)
@pytest.mark.parametrize('H', [16, 32, 64, 128])
def test_cases_hold_what_they_promise(H):
    """The designed list lengths are there (a node in no list; 1, 3, 4, 5, 9 entries in each single list and spread over the four; a
    positive out-list longer than HEAVY_ROW; both self pairs), and the walk's restatement agrees with losses_ref.recon — another
    formulation (pair arrays, torch) of the same loss — on sums, counters and the bound."""
    c, w = _case(H, 'odd')
    ll = SR.list_lengths(c)
    for u, want in c['designed'].items():
        assert tuple(ll[u]) == want, (u, tuple(ll[u]), want)
    assert tuple(ll[0]) == (0, 0, 0, 0) and ll[30][0] > SR.HEAVY_ROW == LR.HEAVY_ROW
    for k in SR.LIST_LENGTHS:
        for lst in range(4):
            assert any(d[lst] == k and sum(d) == k for d in c['designed'].values())
    assert bool(((c['pos'][0] == 50) & (c['pos'][1] == 50)).any()) and bool(((c['neg'][0] == 51) & (c['neg'][1] == 51)).any())
    for size, wp, wn in CASES:
        c, w = _case(H, size, wp, wn)
        r = LR.recon(c['st'], c['pos'], c['neg'])
        for k in range(2):
            assert abs(w['sums'][k] - float(r['sums'][k])) <= 1e-12 * max(1.0, abs(w['sums'][k]))
            assert abs(w['bounds'][k] - (r['sum_bounds'][k] + 1e-12 * abs(float(r['sums'][k])))) <= 1e-9 * max(w['bounds'][k], 1e-30)
        assert w['counts'] == r['counts']
        assert (c['pos'].shape[1] == 0) == (not wp) and (c['neg'].shape[1] == 0) == (not wn)
    m = SR.build_marginal(H)
    assert float(m['margin'].max()) < 1.0 and m['pos'].shape[1] == m['neg'].shape[1] == m['N'] // 2


# ================================================================================================ through the C ABI
def _inputs(c, dev):
    from deepgate import sampling
    from deepgate.graph_plan import GraphPlan
    assert GraphPlan.HEAVY_ROW == SR.HEAVY_ROW
    st, pos, neg = c['st'].to(dev), c['pos'].to(dev), c['neg'].to(dev)
    plan = GraphPlan(pos, c['N'])
    return st, pos, neg, plan, sampling.bucket_negatives(neg, c['N']).csr


def _heavy(plan):
    heavy = [(0, plan.heavy_segments(True), plan.out_dst), (1, plan.heavy_segments(False), plan.in_src)]
    return heavy, (plan.HEAVY_ROW if any(hv is not None for _, hv, _ in heavy) else 0)


def _old_rows(H, N, st, plan, neg_csr, Ep, En, g):
    """mgv_recon_loss_bwd_csr + mgv_recon_heavy_lists at the device scalar g, into NaN-filled rows."""
    from deepgate import _hip, ops
    ptr = _hip.ptr
    out = torch.full_like(st, float('nan'))
    gd = torch.tensor([g], dtype=F32, device=st.device)
    heavy, skip = _heavy(plan)
    _hip.call('mgv_recon_loss_bwd_csr', H, N, ptr(st), ptr(st[:, H:]), 2 * H, ptr(plan.out_ptr), ptr(plan.out_dst), ptr(plan.in_ptr),
              ptr(plan.in_src), Ep, *[ptr(x) for x in neg_csr], En, ptr(gd), ptr(out), ptr(out[:, H:]), skip)
    for which, hv, lst in heavy:
        if hv is not None:
            pw = ops.workspace(hv['S'] * H, st.device)
            _hip.call('mgv_recon_heavy_lists', H, ptr(st), ptr(st[:, H:]), 2 * H, Ep, ptr(gd), hv['K'], ptr(hv['nodes']), ptr(hv['node_seg_ptr']),
                      hv['S'], ptr(hv['seg_node']), ptr(hv['seg_e0']), ptr(hv['seg_e1']), ptr(lst), which, ptr(pw), ptr(out[:, H:]) if which else ptr(out))
    return out, skip


def _step(H, N, st, plan, neg_csr, Ep, En, scale):
    """The one-walk entries -> (rows written into NaN, sums float64 [2], counts int64 [4])."""
    from deepgate import _hip, ops
    ptr = _hip.ptr
    dev = st.device
    out = torch.full_like(st, float('nan'))
    sums, counts = torch.zeros(2, dtype=F64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
    ws = ops.sum_ws(dev)
    heavy, skip = _heavy(plan)
    _hip.call('mgv_recon_step_csr', H, N, ptr(st), ptr(st[:, H:]), 2 * H, ptr(plan.out_ptr), ptr(plan.out_dst), ptr(plan.in_ptr), ptr(plan.in_src),
              Ep, *[ptr(x) for x in neg_csr], En, scale, ptr(sums), ptr(counts), ptr(out), ptr(out[:, H:]), skip, ptr(ws), ws.numel())
    for which, hv, lst in heavy:
        if hv is not None:
            pw = ops.workspace(hv['S'] * H, dev)
            _hip.call('mgv_recon_step_heavy_lists', H, ptr(st), ptr(st[:, H:]), 2 * H, Ep, scale, hv['K'], ptr(hv['nodes']), ptr(hv['node_seg_ptr']),
                      hv['S'], ptr(hv['seg_node']), ptr(hv['seg_e0']), ptr(hv['seg_e1']), ptr(lst), which, ptr(pw),
                      ptr(out[:, H:]) if which else ptr(out), ptr(sums), ptr(counts), ptr(ws), ws.numel())
    return out, sums, counts


def _fwd(H, st, pos, neg):
    """mgv_recon_loss_fwd on the pair arrays -> (sums, counts)."""
    from deepgate import _hip, ops
    ptr = _hip.ptr
    dev = st.device
    sums, counts = torch.zeros(2, dtype=F64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
    ws = ops.sum_ws(dev)
    _hip.call('mgv_recon_loss_fwd', H, ptr(st), ptr(st[:, H:]), 2 * H, ptr(pos[0].contiguous()), ptr(pos[1].contiguous()), pos.shape[1],
              ptr(neg[0].contiguous()), ptr(neg[1].contiguous()), neg.shape[1], ptr(sums), ptr(counts), None, ptr(ws), ws.numel())
    return sums, counts


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=IDS)
@pytest.mark.parametrize('H', [16, 32, 64, 128])
def test_step_entries_against_old_entries_and_float64(H, case):
    dev = _dev()
    size, wp, wn = case
    c, w = _case(H, size, wp, wn)
    N = c['N']
    st, pos, neg, plan, neg_csr = _inputs(c, dev)
    Ep, En = pos.shape[1], neg.shape[1]
    f_sums, f_counts = _fwd(H, st, pos, neg)
    for scale in (1.0, 0.25):
        want, skip = _old_rows(H, N, st, plan, neg_csr, Ep, En, scale)
        assert (skip > 0) == (size != 'one' and wp)                      # the heavy entry carries loss terms where there are positives
        rows, sums, counts = _step(H, N, st, plan, neg_csr, Ep, En, scale)
        assert bool(torch.isfinite(rows).all()), 'rows kept their NaN: %s' % torch.nonzero(~torch.isfinite(rows).all(dim=1)).reshape(-1)[:8].tolist()
        assert torch.equal(rows, want)
        assert counts.tolist() == f_counts.tolist()
        if w['near'] == 0:
            assert counts.tolist() == w['counts']
        assert int(counts.sum()) == Ep + En                             # every pair exactly once
        err = [abs(float(sums[k]) - w['sums'][k]) for k in range(2)]
        gap = [abs(float(sums[k]) - float(f_sums[k])) for k in range(2)]
        print('recon step H=%d %s N=%d E=%d+%d scale=%g: sums err %.3g %.3g (bounds %.3g %.3g)  against the pair pass %.3g %.3g'
              % (H, IDS[CASES.index(case)], N, Ep, En, scale, err[0], err[1], w['bounds'][0], w['bounds'][1], gap[0], gap[1]))
        for k in range(2):
            assert err[k] <= w['bounds'][k] and gap[k] <= 2 * w['bounds'][k]
        again = _step(H, N, st, plan, neg_csr, Ep, En, scale)
        assert torch.equal(again[0], rows) and torch.equal(again[1], sums) and torch.equal(again[2], counts)
    if not wp:
        assert float(sums[0]) == 0.0
    if not wn:
        assert float(sums[1]) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize('H', [16, 32, 64, 128])
def test_counters_on_scores_that_are_rounding_noise(H):
    """Every score of this case is a few last bits around 0 (recon_step_ref.build_marginal; asserted: below one float32 rounding of
    the dot product's terms), so `p > 0.5` goes with the way the score's roundings fall.  The walk's gradient score is contracted into
    fmas, the pair pass's is not: counting hits on the former disagreed with mgv_recon_loss_fwd on one of 13.1 M pairs of the benchmark
    batch.  The walk therefore decides on a score formed the pair pass's way (dot4_plain), and must agree on EVERY pair here; so must
    the rows with the old walk, whose score stays the contracted one."""
    dev = _dev()
    c = SR.build_marginal(H)
    assert float(c['margin'].max()) < 1.0
    N = c['N']
    st, pos, neg, plan, neg_csr = _inputs(c, dev)
    Ep, En = pos.shape[1], neg.shape[1]
    f_sums, f_counts = _fwd(H, st, pos, neg)
    rows, sums, counts = _step(H, N, st, plan, neg_csr, Ep, En, 1.0)
    print('marginal H=%d: counters %s (pair pass %s)' % (H, counts.tolist(), f_counts.tolist()))
    assert min(f_counts.tolist()) > 0                                   # hits and misses on both halves: the decisions do vary
    assert counts.tolist() == f_counts.tolist()
    assert torch.equal(rows, _old_rows(H, N, st, plan, neg_csr, Ep, En, 1.0)[0])
    # the same float terms on both routes (the pair pass holds at most one per thread here: nothing is added in float), in double
    for k in range(2):
        assert abs(float(sums[k]) - float(f_sums[k])) <= 1e-12 * abs(float(f_sums[k]))


@pytest.mark.gpu
@pytest.mark.parametrize('H', [16, 64])
def test_rows_rescale_unless(H):
    """g == expect_scale: the rows keep their bits.  g = 0.5 * expect_scale: they equal the old route's rows at that g within 1 ulp
    per entry — the new route takes one extra rounding (the product with g / expect_scale, where the old route rounds once with g
    inside the coefficient; a factor of exactly 1/2 even commutes with every rounding short of the subnormals)."""
    dev = _dev()
    from deepgate import _hip
    ptr = _hip.ptr
    c, _ = _case(H, 'odd')
    N = c['N']
    st, pos, neg, plan, neg_csr = _inputs(c, dev)
    Ep, En = pos.shape[1], neg.shape[1]
    for scale in (1.0, 0.25):
        rows = _step(H, N, st, plan, neg_csr, Ep, En, scale)[0]
        keep = rows.clone()
        _hip.call('mgv_rows_rescale_unless', rows.numel(), ptr(rows), ptr(torch.tensor([scale], dtype=F32, device=dev)), scale)
        assert torch.equal(rows, keep)
        g = 0.5 * scale
        _hip.call('mgv_rows_rescale_unless', rows.numel(), ptr(rows), ptr(torch.tensor([g], dtype=F32, device=dev)), scale)
        want = _old_rows(H, N, st, plan, neg_csr, Ep, En, g)[0].cpu().numpy()
        got = rows.cpu().numpy()
        ulp = np.spacing(np.abs(want))
        worst = float((np.abs(got.astype(np.float64) - want) / ulp).max())
        print('rows_rescale_unless H=%d expect=%g g=%g: worst difference %.3g ulp' % (H, scale, g, worst))
        assert worst <= 1.0
    # A factor that commutes with no rounding: g = 0.3 through the real rows.  Per entry, with u = 2^-24, T = sum_k |c_k v_k| and n the
    # row's list entries: either route rounds each coefficient four times on the way from g (g / E, * p, * (1 - p), the division: 4 u T)
    # and each partial sum once (n u T), the new route once more for g / expect and once for the product (2 u T) — (10 + 2 n) u T in
    # all, to first order; T <= S, the row's scale from the float64 reference (sum |c_k| max |v_k|).  A heavy list's row passes through
    # up to 64 lane-group partials, its segments and the row it is added to: n + 70 there.  A factor applied the wrong way round
    # (expect / g) or twice is of order T.
    g = LR.f32(0.3)
    rows = _step(H, N, st, plan, neg_csr, Ep, En, 1.0)[0]
    _hip.call('mgv_rows_rescale_unless', rows.numel(), ptr(rows), ptr(torch.tensor([g], dtype=F32, device=dev)), 1.0)
    want = _old_rows(H, N, st, plan, neg_csr, Ep, En, g)[0].cpu().to(F64)
    S = LR.recon(c['st'], c['pos'], c['neg'], gscale=g)['S']
    ll = torch.from_numpy(SR.list_lengths(c)).to(F64)
    worst = 0.0
    for half, sl, n in ((0, slice(0, H), ll[:, 0] + ll[:, 2]), (1, slice(H, 2 * H), ll[:, 1] + ll[:, 3])):
        n = torch.where(n > SR.HEAVY_ROW, n + 70, n)
        err = (rows.cpu().to(F64)[:, sl] - want[:, sl]).abs().amax(dim=1)
        bound = (10 + 2 * n) * U24 * S[:, half]
        assert bool((err[bound == 0] == 0).all())
        live = bound > 0
        worst = max(worst, float((err[live] / bound[live]).max()))
    moved = float(((rows.cpu().to(F64) - want).abs().amax(dim=1) > 0).double().mean())
    print('rows_rescale_unless H=%d expect=1 g=0.3: worst row error / bound %.3g; %.0f %% of the rows differ from the old route in some bit' % (H, worst, 100 * moved))
    assert worst <= 1.0
    # a length that is no multiple of four, and a factor that is no power of two
    x = torch.arange(1, 11, dtype=F32, device=dev) / 7
    y = x.clone()
    _hip.call('mgv_rows_rescale_unless', 10, ptr(y), ptr(torch.tensor([3.0], dtype=F32, device=dev)), 0.7)
    f = np.float32(3.0) / np.float32(0.7)
    assert np.array_equal(y.cpu().numpy(), x.cpu().numpy() * f)
    with pytest.raises(_hip.HipLibraryError):
        _hip.call('mgv_rows_rescale_unless', 10, ptr(y), ptr(torch.tensor([3.0], dtype=F32, device=dev)), 0.0)


# ================================================================================================ through ops
def _ops_run(c, dev, monkeypatch, one_pass, want_pred=False, upstream=1.0, expect_scale=1.0, no_grad=False):
    """-> (loss, counts, pred, gradient of st or None, the launcher names the call used)."""
    from deepgate import _hip, ops
    monkeypatch.setenv('MGV_RECON_ONE_PASS', '1' if one_pass else '0')
    st, pos, neg, plan, neg_csr = _inputs(c, dev)
    x = st.clone().requires_grad_(True)
    old = _hip.profile(True)
    try:
        if no_grad:
            with torch.no_grad():
                loss, counts, pred = ops.ReconLossFn.apply(x, pos, neg, want_pred, plan, neg_csr, expect_scale)
        else:
            loss, counts, pred = ops.ReconLossFn.apply(x, pos, neg, want_pred, plan, neg_csr, expect_scale)
            (loss * upstream).backward()
    finally:
        names = set(_hip.profile(False) or ())
        _hip._profile = old
    return loss.detach(), counts, pred, x.grad, names


@pytest.mark.gpu
@pytest.mark.parametrize('H', [16, 64])
def test_ops_takes_the_walk_for_a_training_step_only(H, monkeypatch):
    dev = _dev()
    c, w = _case(H, 'odd')
    r = LR.recon(c['st'], c['pos'], c['neg'])
    Ep, En = c['pos'].shape[1], c['neg'].shape[1]
    l0, c0, p0, g0, n0 = _ops_run(c, dev, monkeypatch, False)
    l1, c1, p1, g1, n1 = _ops_run(c, dev, monkeypatch, True)
    assert 'mgv_recon_step_csr' in n1 and 'mgv_recon_step_heavy_lists' in n1 and 'mgv_rows_rescale_unless' in n1
    assert not n1 & {'mgv_recon_loss_fwd', 'mgv_recon_loss_bwd_csr', 'mgv_recon_heavy_lists'}
    assert {'mgv_recon_loss_fwd', 'mgv_recon_loss_bwd_csr'} <= n0 and not any('step' in n or 'rescale' in n for n in n0)
    b_loss = r['loss_bound'] + 1e-12 * abs(float(r['loss'])) + 2 * U24 * abs(float(r['loss']))      # the sums' bound as a mean, two float32 roundings
    print('ops H=%d: loss %.9g one walk, %.9g pair pass, float64 %.9g (bound %.3g)' % (H, float(l1), float(l0), float(r['loss']), b_loss))
    assert abs(float(l1) - float(l0)) <= b_loss and abs(float(l1) - float(r['loss'])) <= b_loss
    assert c1.tolist() == c0.tolist() and p1.numel() == 0 and p0.numel() == 0
    assert torch.equal(g1, g0)                                          # upstream 1.0 = expect_scale: the rows as the walk left them
    l2, c2, _, g2, _ = _ops_run(c, dev, monkeypatch, True)
    assert torch.equal(l2, l1) and torch.equal(c2, c1) and torch.equal(g2, g1)
    # an upstream gradient other than the announced one: mended on the device, exactly for a power of two
    _, _, _, g3, n3 = _ops_run(c, dev, monkeypatch, True, upstream=0.5)
    assert 'mgv_recon_step_csr' in n3 and torch.equal(g3, _ops_run(c, dev, monkeypatch, False, upstream=0.5)[3])
    # the announced one, not 1: no rescale happens (bit-identical to the pair-pass route's walk at 0.25)
    _, _, _, g4, _ = _ops_run(c, dev, monkeypatch, True, upstream=0.25, expect_scale=0.25)
    assert torch.equal(g4, _ops_run(c, dev, monkeypatch, False, upstream=0.25)[3])
    # want_pred or no_grad: the old kernels, whatever the switch says
    lp, cp, pp, gp, np_ = _ops_run(c, dev, monkeypatch, True, want_pred=True)
    assert 'mgv_recon_loss_fwd' in np_ and 'mgv_recon_step_csr' not in np_
    assert pp.numel() == Ep + En and torch.equal(lp, l0) and torch.equal(cp, c0) and torch.equal(gp, g0)
    assert int(pp.sum()) == int(c0[0] + c0[1])
    ln, cn, pn, gn, nn = _ops_run(c, dev, monkeypatch, True, no_grad=True)
    assert nn == {'mgv_recon_loss_fwd'} and gn is None and torch.equal(ln, l0) and torch.equal(cn, c0)
    # no plan / no negative CSR, or a zero weight: the old kernels as well
    from deepgate import _hip, ops
    st, pos, neg, plan, neg_csr = _inputs(c, dev)
    for args in ((None, None), (plan, None), (plan, neg_csr, 0.0)):
        x = st.clone().requires_grad_(True)
        _hip.profile(True)
        loss = ops.ReconLossFn.apply(x, pos, neg, False, *args)[0]
        names = set(_hip.profile(False))
        assert 'mgv_recon_loss_fwd' in names and 'mgv_recon_step_csr' not in names and loss.requires_grad
