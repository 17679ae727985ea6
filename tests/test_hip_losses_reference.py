"""The decoder, reconstruction-loss, functional-loss, reparameterisation / KL, confusion and Adam kernels (csrc/losses.hip,
csrc/optim.hip), each driven on its own through deepgate.ops — and through the C ABI where the caller's allocation would hide a
defect — against the float64 restatements of tests/losses_ref.py (pinned on the CPU by tests/test_losses_spec.py, which also
asserts the properties of the input builders used here).

Tolerances.  None is taken from what the device produced.  Forward quantities carry bounds DERIVED from the reference's data and
float32 rounding (stated where they are asserted).  Gradients are compared ROW BY ROW against each row's own scale (the sum of the
magnitudes of its terms, from the reference): max|d[row] - ref[row]| <= tau * S[row], with tau = 8 * max(r32, 2^-23) where r32 is
the worst such ratio of the same torch formula run in float32 on the CPU on the same inputs — 8 because the device uses one-ulp
exp / reciprocal instructions and another summation order where torch rounds a libm sigmoid.  A lost, doubled or stale list
entry is of order 1 on its row's scale.  Every test prints the device's measured figure beside its bound."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import losses_ref as LR  # noqa: E402

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
U24 = 2.0 ** -24
G_UP = 1.7                      # upstream gradient of the losses (!= 1)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _tau(r32):
    return 8 * max(r32, 2.0 ** -23)


# ================================================================================================ decoder / reconstruction
@functools.lru_cache(maxsize=None)      # (the forward, backward and ABI tests share a case's reference: ~0.5 GB for all of them)
def _recon_ref(H, size, wide=False, want_pos=True, want_neg=True):
    """(case, float64 reference at upstream gradient G_UP, r32 = worst row ratio of the float32 CPU restatement)."""
    c = LR.recon_case(H, size, wide=wide, want_pos=want_pos, want_neg=want_neg)
    g = LR.f32(G_UP)
    r64 = LR.recon(c['st'], c['pos'], c['neg'], gscale=g)
    r32 = LR.recon(c['st'], c['pos'], c['neg'], gscale=g, dtype=F32)
    return c, r64, _recon_ratio(r32['grad'], r64, H)


def _recon_ratio(grad, r64, H):
    return max(LR.row_ratio(grad[:, :H], r64['grad'][:, :H], r64['S'][:, 0]), LR.row_ratio(grad[:, H:], r64['grad'][:, H:], r64['S'][:, 1]))


def _recon_inputs(c, dev, route):
    """(st, pos, neg, plan, neg_csr) on the device for a backward route: 'atomic' (k_recon_bwd_rows twice), 'plan' (k_recon_bwd_pull +
    rows for the negatives), 'csr' (k_recon_bwd_pull2, plus the heavy-list kernels when the plan has heavy lists)."""
    from deepgate import sampling
    from deepgate.graph_plan import GraphPlan
    assert (GraphPlan.HEAVY_ROW, GraphPlan.HEAVY_SEG) == (LR.HEAVY_ROW, LR.HEAVY_SEG)
    st, pos, neg = c['st'].to(dev), c['pos'].to(dev), c['neg'].to(dev)
    plan = GraphPlan(pos, c['N']) if route in ('plan', 'csr') else None
    neg_csr = sampling.bucket_negatives(neg, c['N']).csr if route == 'csr' else None
    return st, pos, neg, plan, neg_csr


def _recon_backward(c, dev, route):
    from deepgate import ops
    st, pos, neg, plan, neg_csr = _recon_inputs(c, dev, route)
    x = st.clone().requires_grad_(True)
    loss, counts, pred = ops.ReconLossFn.apply(x, pos, neg, True, plan, neg_csr)
    (loss * G_UP).backward()
    return loss.detach(), counts, pred, x.grad, plan


SIZES = ('n1', 'n15', 'n16', 'n17', 'n127', 'n129', 'xcd_short', 'xcd', 'odd', 'cap')


@pytest.mark.parametrize('wide', [False, True])
@pytest.mark.parametrize('H', [16, 32, 64, 128])
def test_decoder_and_recon_forward(H, wide):
    """mgv_edge_dot_fwd (raw, sigmoid) per edge and mgv_recon_loss_fwd (loss, the two sums, pred_bin, the four counters).
    Bounds, from the reference alone: |raw| error <= H 2^-24 sum_i |s_i t_i| (a length-H float32 sum in any order); |p| error <= dq =
    4 * 2^-24 + p (1 - p) * that (one rounding each for exp, add, reciprocal and one to spare, the dot product's error through the
    sigmoid's slope); each sum's error <= sum(dq / q), q = p or 1 - p, plus the double accumulation (1e-12 relative); the loss adds
    one rounding to float32.  Decisions and counters: exact — the builder keeps every score outside (-1e-3, 1e-3) except exact zeros
    (float32 dot-product rounding at H = 128 and sum |s_i t_i| <= 14 is 1.1e-4), and an exact zero gives p = 0.5: not a hit."""
    dev = _dev()
    from deepgate import _hip, ops
    for size in (('odd',) if wide else ('n1', 'n17', 'n129', 'xcd_short', 'odd', 'cap')):
        c, r64, _ = _recon_ref(H, size, wide)
        st, pos, neg = c['st'].to(dev), c['pos'].to(dev), c['neg'].to(dev)
        Ep, En = pos.shape[1], neg.shape[1]
        s, t = st[:, :H].contiguous(), st[:, H:].contiguous()
        ei = torch.cat([pos, neg], dim=1)
        raw = ops.edge_dot(s, t, ei, sigmoid=False).cpu().to(F64)
        p = ops.edge_dot(s, t, ei, sigmoid=True).cpu().to(F64)
        raw_b = H * U24 * r64['absdot'] + 1e-37
        w_raw, w_p = float(((raw - r64['raw']).abs() / raw_b).max()), float(((p - r64['p']).abs() / r64['dq']).max())
        loss, counts, pred = ops.ReconLossFn.apply(st, pos, neg, True, None, None)
        # the two sums through the ABI (ops folds them into the float32 loss)
        sums = torch.zeros(2, dtype=F64, device=dev)
        cnt2 = torch.zeros(4, dtype=torch.int64, device=dev)
        ws = ops.sum_ws(dev)
        _hip.call('mgv_recon_loss_fwd', H, _hip.ptr(st), _hip.ptr(st[:, H:]), 2 * H, _hip.ptr(pos[0].contiguous()), _hip.ptr(pos[1].contiguous()), Ep,
                  _hip.ptr(neg[0].contiguous()), _hip.ptr(neg[1].contiguous()), En, _hip.ptr(sums), _hip.ptr(cnt2), None, _hip.ptr(ws), ws.numel())
        sums = sums.cpu()
        e_sum = [abs(float(sums[k]) - float(r64['sums'][k])) for k in range(2)]
        b_sum = [r64['sum_bounds'][k] + 1e-12 * abs(float(r64['sums'][k])) for k in range(2)]
        e_loss = abs(float(loss) - float(r64['loss']))
        b_loss = r64['loss_bound'] + 1e-12 * abs(float(r64['loss'])) + 2 * U24 * abs(float(r64['loss']))
        print('recon fwd H=%d %s%s N=%d E=%d+%d: raw err/bound %.3g  p err/dq %.3g  sums err %.3g %.3g (bounds %.3g %.3g)  loss err %.3g (bound %.3g)'
              % (H, size, ' wide' if wide else '', c['N'], Ep, En, w_raw, w_p, e_sum[0], e_sum[1], b_sum[0], b_sum[1], e_loss, b_loss))
        assert w_raw <= 1.0 and w_p <= 1.0
        assert e_sum[0] <= b_sum[0] and e_sum[1] <= b_sum[1] and e_loss <= b_loss
        assert torch.equal(pred.cpu(), r64['pred'])
        assert counts.cpu().tolist() == r64['counts'] and cnt2.cpu().tolist() == r64['counts']
        zero = r64['raw'] == 0
        if bool(zero.any()):
            assert bool((p[zero] == 0.5).all()) and not bool(pred.cpu()[zero].any())


def _routes(H):
    return ('csr',) if H == 128 else ('atomic', 'plan', 'csr')


@pytest.mark.parametrize('size', SIZES)
@pytest.mark.parametrize('H', [16, 32, 64, 128])
def test_recon_backward_each_route_against_float64(H, size):
    """Every backward route on its own against the float64 gradient, row by row on the row's own scale (module docstring); the
    loss, counters and decisions of the same call once more.  Small sizes run the CSR pull with skip_len = 0, the designed ones
    (N >= 4096: list totals 0 .. 65, hubs of 512 / 513 / thousands, heavy on one side only) with skip_len = HEAVY_ROW and the
    heavy-list kernels."""
    dev = _dev()
    c, r64, r32 = _recon_ref(H, size)
    tau = _tau(r32)
    for route in _routes(H):
        loss, counts, pred, grad, plan = _recon_backward(c, dev, route)
        ratio = _recon_ratio(grad.cpu(), r64, H)
        heavy = plan is not None and route == 'csr' and (plan.heavy_segments(True) is not None or plan.heavy_segments(False) is not None)
        print('recon bwd H=%d %s N=%d route=%s%s: worst row ratio %.3g  (float32 restatement %.3g, tau %.3g)'
              % (H, size, c['N'], route, ' +heavy' if heavy else '', ratio, r32, tau))
        assert ratio <= tau, (route, ratio, tau)
        assert counts.cpu().tolist() == r64['counts'] and torch.equal(pred.cpu(), r64['pred'])
        if route == 'csr':
            assert heavy == (c['N'] >= LR.DESIGNED_MIN_N)
            again = _recon_backward(c, dev, route)[3]
            assert torch.equal(again, grad)                              # no atomics on this route: bit-reproducible


def _csr_abi(H, N, s, t, ld, plan, neg_csr, Ep, En, g, ds, dt):
    """The CSR route straight through the C ABI, as ops.ReconLossFn.backward drives it, into caller-owned ds / dt."""
    from deepgate import _hip, ops
    ptr = _hip.ptr
    heavy = [(0, plan.heavy_segments(True), plan.out_dst), (1, plan.heavy_segments(False), plan.in_src)]
    skip = plan.HEAVY_ROW if any(hv is not None for _, hv, _ in heavy) else 0
    _hip.call('mgv_recon_loss_bwd_csr', H, N, ptr(s), ptr(t), ld, ptr(plan.out_ptr), ptr(plan.out_dst), ptr(plan.in_ptr), ptr(plan.in_src), Ep,
              *[ptr(x) for x in neg_csr], En, ptr(g), ptr(ds), ptr(dt), skip)
    for which, hv, lst in heavy:
        if hv is not None:
            pw = ops.workspace(hv['S'] * H, s.device)
            _hip.call('mgv_recon_heavy_lists', H, ptr(s), ptr(t), ld, Ep, ptr(g), hv['K'], ptr(hv['nodes']), ptr(hv['node_seg_ptr']), hv['S'],
                      ptr(hv['seg_node']), ptr(hv['seg_e0']), ptr(hv['seg_e1']), ptr(lst), which, ptr(pw), ptr(dt) if which else ptr(ds))
    return skip


@pytest.mark.parametrize('size', ['n17', 'xcd_short', 'xcd', 'cap'])
@pytest.mark.parametrize('H', [16, 32, 64, 128])
def test_csr_route_owns_every_row(H, size):
    """mgv_recon_loss_bwd_csr / mgv_recon_heavy_lists write into NaN-filled ds / dt: every row must come out finite and bit-equal to
    the ops result (the kernel, not the allocator, owns every row) — in the product's interleaved [N, 2H] layout and with separate
    s, t of leading dimension H and H + 4."""
    dev = _dev()
    c, r64, _ = _recon_ref(H, size)
    N = c['N']
    st, pos, neg, plan, neg_csr = _recon_inputs(c, dev, 'csr')
    want = _recon_backward(c, dev, 'csr')[3]
    g = torch.tensor([G_UP], dtype=F32, device=dev)
    Ep, En = pos.shape[1], neg.shape[1]
    out = torch.full_like(st, float('nan'))
    _csr_abi(H, N, st, st[:, H:], 2 * H, plan, neg_csr, Ep, En, g, out, out[:, H:])
    assert bool(torch.isfinite(out).all()), 'rows kept their NaN: %s' % torch.nonzero(~torch.isfinite(out).all(dim=1)).reshape(-1)[:8].tolist()
    assert torch.equal(out, want)
    for ld in (H, H + 4):
        s, t = torch.full((N, ld), 7.0, device=dev), torch.full((N, ld), -7.0, device=dev)       # the padding is never read
        s[:, :H], t[:, :H] = st[:, :H], st[:, H:]
        ds, dt = torch.full((N, ld), float('nan'), device=dev), torch.full((N, ld), float('nan'), device=dev)
        _csr_abi(H, N, s, t, ld, plan, neg_csr, Ep, En, g, ds, dt)
        assert torch.equal(ds[:, :H], want[:, :H]) and torch.equal(dt[:, :H], want[:, H:])
        assert bool(torch.isnan(ds[:, H:]).all()) and bool(torch.isnan(dt[:, H:]).all())        # ... and never written


@pytest.mark.parametrize('H', [16, 64, 128])
@pytest.mark.parametrize('side', ['pos_only', 'neg_only'])
def test_one_sided_edge_sets(H, side):
    """Ep = 0 with negatives only, En = 0 with positives only, forward and every backward route that accepts them.  An empty half
    contributes 0 (ops.ReconLossFn: sums / max(E, 1)), not the NaN of torch's mean over nothing."""
    dev = _dev()
    kw = dict(want_pos=(side == 'pos_only'), want_neg=(side == 'neg_only'))
    for size in ('n17', 'xcd'):
        c, r64, r32 = _recon_ref(H, size, False, kw['want_pos'], kw['want_neg'])
        assert (c['pos'].shape[1] == 0) == (side == 'neg_only') and (c['neg'].shape[1] == 0) == (side == 'pos_only')
        tau = _tau(r32)
        for route in _routes(H):
            loss, counts, pred, grad, _ = _recon_backward(c, dev, route)
            ratio = _recon_ratio(grad.cpu(), r64, H)
            e_loss = abs(float(loss) - float(r64['loss']))
            print('recon %s H=%d %s route=%s: loss err %.3g (bound %.3g)  worst row ratio %.3g (tau %.3g)'
                  % (side, H, size, route, e_loss, r64['loss_bound'], ratio, tau))
            assert bool(torch.isfinite(loss)) and e_loss <= r64['loss_bound'] + 2 * U24 * abs(float(r64['loss']))
            assert ratio <= tau
            assert counts.cpu().tolist() == r64['counts'] and torch.equal(pred.cpu(), r64['pred'])


def test_atomic_route_refuses_h128_before_it_writes():
    """The one-float-per-lane atomic kernels stop at H = 64.  With a plan the launcher used to run the pull half at H = 128 and THEN
    return MGV_EUNSUPPORTED (a half-written gradient behind an exception); it now refuses before anything is launched: the
    zero-filled gradient stays zero."""
    dev = _dev()
    from deepgate import _hip
    from deepgate._hip import HipLibraryError
    c, _, _ = _recon_ref(128, 'n129')
    for route in ('atomic', 'plan'):
        with pytest.raises(HipLibraryError):
            _recon_backward(c, dev, route)
    st, pos, neg, plan, _ = _recon_inputs(c, dev, 'plan')
    H, ptr = 128, _hip.ptr
    out = torch.zeros_like(st)
    g = torch.tensor([G_UP], dtype=F32, device=dev)
    with pytest.raises(HipLibraryError):
        _hip.call('mgv_recon_loss_bwd', H, c['N'], ptr(st), ptr(st[:, H:]), 2 * H, ptr(pos[0].contiguous()), ptr(pos[1].contiguous()), pos.shape[1],
                  ptr(plan.out_ptr), ptr(plan.out_dst), ptr(plan.in_ptr), ptr(plan.in_src), ptr(neg[0].contiguous()), ptr(neg[1].contiguous()),
                  neg.shape[1], ptr(g), ptr(out), ptr(out[:, H:]))
    torch.cuda.synchronize()
    assert not bool(out.any())


# ================================================================================================ functional loss
@functools.lru_cache(maxsize=2)
def _func_ref(H, P, signed):
    c = LR.func_case(H, P, signed=signed)
    g = LR.f32(G_UP)
    add = torch.from_numpy(np.random.Generator(np.random.PCG64(P)).standard_normal((c['N'], H)).astype(np.float32) * 1e-3)
    f64 = LR.func(c['hf'], c['pairs'], c['tt'], gscale=g)
    f32 = LR.func(c['hf'], c['pairs'], c['tt'], gscale=g, dtype=F32)
    return c, add, f64, LR.row_ratio(f32['grad'], f64['grad'], f64['S'])


class _Cache:
    pass


@pytest.mark.parametrize('P', LR.FUNC_P)
@pytest.mark.parametrize('H', [16, 32, 64])
def test_func_loss_forward_and_each_backward_route(H, P):
    """mgv_func_loss_fwd: dis per pair (<= 4 * 2^-24 + H 2^-24 sum |x_i y_i| / (n_x n_y)), the seven sums (1e-6 of the sum of their
    terms' magnitudes: double sums of float terms; the sign sum exactly — the builder keeps every |zd - zt| >= 1e-4 at every size,
    so the L1 signs are compared exactly and no sign needs imposing), the loss.  Backward: the atomic route (k_func_bwd), the pull
    route (k_func_bwd_pull), the pull route with `add` (ops.func_loss_passthrough with a second consumer), each row by row against
    float64; rows of nodes in no pair must be exactly zero, or exactly `add`."""
    dev = _dev()
    from deepgate import _hip, ops
    signed = (P % 2 == 1)
    c, add, f64, r32 = _func_ref(H, P, signed)
    tau = _tau(r32)
    N = c['N']
    hf, pairs, tt = c['hf'].to(dev), c['pairs'].to(dev), c['tt'].to(dev)
    # forward through the ABI: dis and the workspace sums
    dis = torch.empty(P, dtype=F32, device=dev)
    ws = torch.zeros(8, dtype=F64, device=dev)
    sw = ops.sum_ws(dev)
    pa, pb = pairs[0].contiguous(), pairs[1].contiguous()
    _hip.call('mgv_func_loss_fwd', H, P, _hip.ptr(hf), _hip.ptr(pa), _hip.ptr(pb), _hip.ptr(tt), 1e-8, _hip.ptr(dis), _hip.ptr(ws), _hip.ptr(sw), sw.numel())
    w_dis = float(((dis.cpu().to(F64) - f64['dis']).abs() / f64['bound_dis']).max())
    sums = ws.cpu()[:7]
    rel = ((sums - f64['sums']).abs() / f64['sums_abs'].clamp_min(1e-300)).tolist()
    print('func fwd H=%d P=%d: dis err/bound %.3g  sums rel err %s' % (H, P, w_dis, ' '.join('%.2g' % v for v in rel)))
    assert w_dis <= 1.0
    assert max(rel) <= 1e-6 and float(sums[5]) == float(f64['sums'][5])
    cnt = (torch.bincount(c['pairs'][0], minlength=N) + torch.bincount(c['pairs'][1], minlength=N)).to(F64)      # pair memberships per row
    used = cnt > 0
    results = {}
    for route in ('atomic', 'pull', 'pull_add'):
        x = hf.clone().requires_grad_(True)
        if route == 'atomic':
            loss = ops.func_loss(x, pairs, tt)
            (loss * G_UP).backward()
        elif route == 'pull':
            loss = ops.func_loss(x, pairs, tt, cache=_Cache())
            (loss * G_UP).backward()
        else:
            loss, x2 = ops.func_loss_passthrough(x, pairs, tt, cache=_Cache())
            (loss * G_UP + (x2 * add.to(dev)).sum()).backward()
        e_loss = abs(float(loss.detach()) - float(f64['loss']))
        got = x.grad.cpu()
        if route == 'pull_add':
            # the kernel starts a row's sum from `add` and adds the row's 2 * cnt terms to it one fused multiply-add at a time: beside
            # tau * S, each of those roundings is at most 2^-24 of the running sum, itself at most max|add[row]| + S[row] (derived:
            # sequential float32 summation; nothing here comes from the device)
            a_max = add.to(F64).abs().amax(dim=1)
            bound = tau * f64['S'] + (2 * cnt + 1) * U24 * (a_max + f64['S'])
            ratio = LR.row_ratio(got, f64['grad'] + add.to(F64), bound) * tau          # in units of tau, like the other routes
        else:
            ratio = LR.row_ratio(got, f64['grad'], f64['S'])
        print('func bwd H=%d P=%d route=%s: loss err %.3g  worst row ratio %.3g (float32 restatement %.3g, tau %.3g)' % (H, P, route, e_loss, ratio, r32, tau))
        assert e_loss <= 1e-6 * float(f64['sums_abs'][4]) / P + 2 * U24 * abs(float(f64['loss']))
        assert ratio <= tau, (route, ratio, tau)
        if bool((~used).any()):
            idle = got[~used]
            assert torch.equal(idle, add[~used]) if route == 'pull_add' else not bool(idle.any())
        results[route] = x.grad
    # the pull route straight through the ABI into a NaN-filled dhf
    lists = ops.pair_lists(pairs, N)
    g = torch.tensor([G_UP], dtype=F32, device=dev)
    out = torch.full_like(hf, float('nan'))
    _hip.call('mgv_func_loss_bwd_csr', H, N, P, _hip.ptr(hf), _hip.ptr(pa), _hip.ptr(pb), _hip.ptr(tt), _hip.ptr(dis), 1e-8, _hip.ptr(ws), _hip.ptr(g),
              *[_hip.ptr(t) for t in lists], None, _hip.ptr(out))
    assert bool(torch.isfinite(out).all()) and torch.equal(out, results['pull'])


def test_func_loss_of_a_constant_target_is_not_a_finite_number():
    """tt constant: zero variance, the reference's loss is NaN (0 / 0); the device must not answer with a finite number."""
    dev = _dev()
    from deepgate import ops
    c = LR.func_case(64, 257)
    tt = torch.full((257,), 0.5)
    hf64 = c['hf'].to(F64)
    a, b = hf64[c['pairs'][0]], hf64[c['pairs'][1]]
    dis = 1 - torch.nn.functional.cosine_similarity(a, b, eps=1e-8)
    ref = torch.nn.functional.l1_loss((dis - dis.mean()) / dis.std(), (tt.to(F64) - 0.5) / tt.to(F64).std())
    assert not bool(torch.isfinite(ref))
    x = c['hf'].to(dev).requires_grad_(True)
    loss = ops.func_loss(x, c['pairs'].to(dev), tt.to(dev), cache=_Cache())
    assert not bool(torch.isfinite(loss))


# ================================================================================================ reparameterisation + KL
def _reparam_inputs(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    mu = (2 * rng.standard_normal(n)).astype(np.float32)
    ls = rng.uniform(-6.0, 3.0, size=n).astype(np.float32)
    eps = rng.standard_normal(n).astype(np.float32)
    gz = rng.standard_normal(n).astype(np.float32)
    return [torch.from_numpy(x) for x in (mu, ls, eps, gz)]


@pytest.mark.parametrize('n', [1, 255, 257, (1 << 20) + 3])
def test_reparam_and_kl_against_float64(n):
    """z, the KL sum and both gradients with a given eps: |dz| <= 8 * 2^-24 (|mu| + e^l |eps|), the gradients likewise on the sum of
    their terms' magnitudes (one-ulp exp, a handful of roundings), the KL sum within 1e-6 of sum 1 + |2 l| + mu^2 + e^(2l) (float
    terms, double sum).  gz and gkl each present and absent, klcoef != 1 (through the ABI; ops.ReparamFn fixes klcoef = 1)."""
    dev = _dev()
    from deepgate import _hip, ops
    ptr = _hip.ptr
    mu, ls, eps, gz = _reparam_inputs(n, n)
    d = [x.to(dev) for x in (mu, ls, eps, gz)]
    z = torch.full((n,), float('nan'), device=dev)
    kl = torch.zeros(1, dtype=F64, device=dev)
    _hip.call('mgv_reparam_fwd', n, ptr(d[0]), ptr(d[1]), ptr(d[2]), 0, None, ptr(z), ptr(kl))
    r = LR.reparam(mu, ls, eps)
    w_z = float(((z.cpu().to(F64) - r['z']).abs() / (8 * U24 * r['z_abs'] + 1e-37)).max())
    e_kl = abs(float(kl.cpu()[0]) - float(r['kl'])) / float(r['kl_abs'])
    print('reparam n=%d: z err / bound %.3g   KL sum rel err %.3g (bound 1e-6)' % (n, w_z, e_kl))
    assert w_z <= 1.0 and e_kl <= 1e-6
    gkl = torch.tensor([0.37], dtype=F32, device=dev)
    for use_gz, use_gkl, klcoef in ((True, True, -0.8), (True, False, 1.0), (False, True, 2.5), (False, False, 1.0)):
        dmu, dls = torch.full((n,), float('nan'), device=dev), torch.full((n,), float('nan'), device=dev)
        _hip.call('mgv_reparam_bwd', n, ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]) if use_gz else None, ptr(gkl) if use_gkl else None, klcoef,
                  ptr(dmu), ptr(dls))
        rb = LR.reparam(mu, ls, eps, gz=gz if use_gz else None, gkl=LR.f32(0.37) if use_gkl else None, klcoef=LR.f32(klcoef))
        w_mu = float(((dmu.cpu().to(F64) - rb['dmu']).abs() / (8 * U24 * rb['dmu_abs'] + 1e-37)).max())
        w_ls = float(((dls.cpu().to(F64) - rb['dls']).abs() / (8 * U24 * rb['dls_abs'] + 1e-37)).max())
        print('   gz %s gkl %s klcoef %g: dmu err / bound %.3g  dlogstd err / bound %.3g' % (use_gz, use_gkl, klcoef, w_mu, w_ls))
        assert w_mu <= 1.0 and w_ls <= 1.0
    # the autograd node: klcoef = 1
    m, l = d[0].clone().requires_grad_(True), d[1].clone().requires_grad_(True)
    zz, kk = ops.ReparamFn.apply(m, l, d[2], 0)
    ((zz * d[3]).sum() + 0.37 * kk).backward()
    rb = LR.reparam(mu, ls, eps, gz=gz, gkl=LR.f32(0.37))
    assert torch.equal(zz, z)
    assert float(((m.grad.cpu().to(F64) - rb['dmu']).abs() / (8 * U24 * rb['dmu_abs'] + 1e-37)).max()) <= 1.0
    assert float(((l.grad.cpu().to(F64) - rb['dls']).abs() / (8 * U24 * rb['dls_abs'] + 1e-37)).max()) <= 1.0


@pytest.mark.parametrize('n', [1, 255, 257, (1 << 20) + 3])
def test_builtin_gaussian_generator_element_by_element(n):
    """eps_out of mgv_reparam_fwd against losses_ref.gauss_from_counter (the hash bit for bit, the uniforms as the kernel forms them,
    Box-Muller in float64).  Floor, derived: u2 is scaled by 2 pi in float32 — an argument error up to 2 pi 2^-24 — times the radius
    <= sqrt(2 * 24 ln 2) = 5.77: 2.2e-6 absolute.  Asserted: 16 x that (the fast cosine and logf near u1 -> 1 are not documented to
    better)."""
    dev = _dev()
    from deepgate import _hip, ops
    ptr = _hip.ptr
    mu, ls, _, _ = _reparam_inputs(n, 5 * n)
    d = [x.to(dev) for x in (mu, ls)]
    outs, zs = [], []
    for seed in (0, 20260101, 20260101, 0xDEADBEEFCAFEF00D):
        e, z = torch.full((n,), float('nan'), device=dev), torch.empty(n, device=dev)
        kl = torch.zeros(1, dtype=F64, device=dev)
        _hip.call('mgv_reparam_fwd', n, ptr(d[0]), ptr(d[1]), None, seed, ptr(e), ptr(z), ptr(kl))
        want = LR.gauss_from_counter(seed, n)
        err = float(np.abs(e.cpu().numpy().astype(np.float64) - want).max())
        print('generator n=%d seed=%#x: worst |eps - ref| %.3g  (floor %.3g, asserted %.3g)' % (n, seed, err, LR.GAUSS_FLOOR, 16 * LR.GAUSS_FLOOR))
        assert err <= 16 * LR.GAUSS_FLOOR
        r = LR.reparam(mu, ls, e.cpu())
        assert float(((z.cpu().to(F64) - r['z']).abs() / (8 * U24 * r['z_abs'] + 1e-37)).max()) <= 1.0      # z uses the eps it reports
        outs.append(e)
        zs.append(z)
    assert torch.equal(outs[1], outs[2])
    if n >= 255:
        assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[3])
    # through ops (eps=None): the same stream
    zz, _ = ops.ReparamFn.apply(d[0], d[1], None, 20260101)
    assert torch.equal(zz, zs[1])


# ================================================================================================ confusion counters
@pytest.mark.parametrize('n', [1, 257, (1 << 24) + 3])
def test_confusion_counters_are_exact(n):
    """mgv_confusion with entries other than 0 / 1 in pred (counted nowhere), and the counters of mgv_recon_loss_fwd at the same
    sizes: per-thread integer counts and double block sums must stay exact past float's integer range (2^24)."""
    dev = _dev()
    from deepgate import ops
    rng = np.random.Generator(np.random.PCG64(n))
    pred = rng.choice(np.array([0, 1, 2, -1], dtype=np.int32), size=n, p=[0.3, 0.6, 0.05, 0.05])
    gt = rng.integers(0, 2, size=n).astype(np.int32)
    got = ops.confusion_counts(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)).cpu().tolist()
    assert got == LR.confusion(pred, gt)
    if n > 1000:
        assert sum(got) < n and got[0] > 1 << 22
        # one counter past 2^24: everything a true positive but one entry that is counted nowhere
        pred[:], gt[:] = 1, 1
        pred[n // 3] = 2
        got = ops.confusion_counts(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)).cpu().tolist()
        assert got == [n - 1, 0, 0, 0] and n - 1 > 1 << 24
    # recon forward: scores from a table over 64 nodes
    N, H = 64, 16
    c = LR.build_recon(N, H, seed=n % 1000)
    st = c['st']
    table = LR.edge_scores(st[:, :H], st[:, H:], torch.stack([torch.arange(N).repeat_interleave(N), torch.arange(N).repeat(N)]), sigmoid=False).reshape(N, N)
    ok = torch.nonzero((table.abs() >= LR.BAND) | (table == 0))                  # pairs whose decision float32 cannot move
    Ep = n - n // 8
    pick = torch.from_numpy(rng.integers(0, ok.shape[0], size=n))
    ei = ok[pick].t().contiguous()
    if n > 1000:
        # TP past 2^24: all positives, all hits but one
        hits, miss = torch.nonzero(table > LR.BAND), torch.nonzero(table < -LR.BAND)
        ei = hits[torch.from_numpy(rng.integers(0, hits.shape[0], size=n + 4))].t().contiguous()
        ei[:, n // 2] = miss[0]
        Ep = n                                               # TP = n - 1 = 2^24 + 2; four negatives behind them
    hit = (table[ei[0], ei[1]] > 0).numpy()
    want = [int(hit[:Ep].sum()), int(hit[Ep:].sum()), int((~hit[Ep:]).sum()), int((~hit[:Ep]).sum())]
    eid = ei.to(dev)
    loss, counts, pb = ops.ReconLossFn.apply(st.to(dev), eid[:, :Ep], eid[:, Ep:], True, None, None)
    assert counts.cpu().tolist() == want and sum(want) == ei.shape[1] and (n < 1000 or want[0] > 1 << 24)
    assert np.array_equal(pb.cpu().numpy().astype(bool), hit)
    assert bool(torch.isfinite(loss))


# ================================================================================================ Adam
LR_ADAM, EPS_ADAM, K_STEPS = 1e-3, 1e-8, 200
_build_adam = functools.lru_cache(maxsize=1)(LR.build_adam)


def _adam_bounds(c, betas, wd, gs, K, first_step=1, m0=None, v0=None):
    """float64 reference on the float32 values the ABI receives, and the reference's float32 self: torch.optim.Adam in float32 on the
    CPU on the same sequence.  -> (ref, figures {p: max |dp|, m, v: max error relative to the element's scale}, bounds):
    bound(p) = max(4 * figure, 8 * 2^-24 * max|p|), bound(m), bound(v) = max(4 * figure, 8 * 2^-24) of the element's scale."""
    n = c['p'].numel()
    m0 = torch.zeros(n) if m0 is None else m0
    v0 = torch.zeros(n) if v0 is None else v0
    ref = LR.adam(c['p'], c['g'][:K], m0, v0, LR.f32(LR_ADAM), (LR.f32(betas[0]), LR.f32(betas[1])), LR.f32(EPS_ADAM), LR.f32(wd), LR.f32(gs), first_step)
    q = torch.nn.Parameter(c['p'].clone())
    opt = torch.optim.Adam([q], lr=LR_ADAM, betas=betas, eps=EPS_ADAM, weight_decay=wd)
    if first_step > 1 or m0.any() or v0.any():
        opt.state[q] = {'step': torch.tensor(float(first_step - 1)), 'exp_avg': m0.clone(), 'exp_avg_sq': v0.clone()}
    for k in range(K):
        q.grad = c['g'][k] * gs
        opt.step()
    st = opt.state[q]
    fig = {'p': float((q.detach().to(F64) - ref['p']).abs().max()),
           'm': _scaled(st['exp_avg'], ref['m'], ref['m_scale']), 'v': _scaled(st['exp_avg_sq'], ref['v'], ref['v_scale'])}
    bounds = {'p': max(4 * fig['p'], 8 * U24 * float(ref['p'].abs().max())), 'm': max(4 * fig['m'], 8 * U24), 'v': max(4 * fig['v'], 8 * U24)}
    return ref, fig, bounds


def _scaled(got, ref, scale):
    """max |got - ref| / scale over the elements with a scale; elements without one (no gradient ever) must be exactly the reference's."""
    err = (got.detach().cpu().to(F64) - ref).abs()
    dead = scale == 0
    assert not bool(err[dead].any())
    return float((err[~dead] / scale[~dead]).max()) if bool((~dead).any()) else 0.0


def _check_adam(tag, p, m, v, ref, fig, bounds):
    got = {'p': float((p.cpu().to(F64) - ref['p']).abs().max()), 'm': _scaled(m, ref['m'], ref['m_scale']), 'v': _scaled(v, ref['v'], ref['v_scale'])}
    print('adam %s: device p %.3g m %.3g v %.3g | float32 torch p %.3g m %.3g v %.3g | bounds p %.3g m %.3g v %.3g'
          % (tag, got['p'], got['m'], got['v'], fig['p'], fig['m'], fig['v'], bounds['p'], bounds['m'], bounds['v']))
    for k in 'pmv':
        assert got[k] <= bounds[k], (tag, k, got[k], bounds[k])


# every combination at n = 257 (one full and one partial workgroup), the other sizes with two opposite configurations each
ADAM_CONFIGS = ([(257, wd, gs, betas) for wd in (0.0, 1e-2) for gs in (1.0, 0.125) for betas in ((0.9, 0.999), (0.5, 0.9))]
                + [(n, *cfg) for n in (1, 255, 100003, 524288 + 5) for cfg in ((1e-2, 0.125, (0.9, 0.999)), (0.0, 1.0, (0.5, 0.9)))])


@pytest.mark.parametrize('n,wd,gs,betas', ADAM_CONFIGS)
def test_adam_200_steps_against_float64(n, wd, gs, betas):
    """ops.adam_step over 200 steps of a fixed gradient sequence (magnitudes 1e-8 .. 1, elements whose gradient is zero throughout —
    v = 0, denom = eps — and elements that wake up after 100 steps): p absolutely, m and v relative to their per-element scales (relative
    to the values themselves they cancel), each within the bound measured from torch.optim.Adam in float32 (see _adam_bounds)."""
    dev = _dev()
    from deepgate import ops
    c = _build_adam(n, K_STEPS, seed=n % 977 + 1)
    ref, fig, bounds = _adam_bounds(c, betas, wd, gs, K_STEPS)
    p, m, v = c['p'].to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    g = c['g'].to(dev)
    for k in range(K_STEPS):
        ops.adam_step(p, g[k], m, v, LR_ADAM, betas, EPS_ADAM, wd, gs, k + 1)
    _check_adam('n=%d wd=%g gs=%g betas=%s' % (n, wd, gs, betas), p, m, v, ref, fig, bounds)
    if wd == 0:
        assert torch.equal(p.cpu()[torch.from_numpy(c['dead'])], c['p'][torch.from_numpy(c['dead'])])      # zero gradient, zero moments: not moved


@pytest.mark.parametrize('step', [10, 1000, 100000])
@pytest.mark.parametrize('wd', [0.0, 1e-2])
def test_adam_single_step_from_nonzero_moments(step, wd):
    dev = _dev()
    from deepgate import ops
    n = 100003
    c = LR.build_adam(n, 2, seed=step)
    rng = np.random.Generator(np.random.PCG64(step + 1))
    m0 = torch.from_numpy((c['g'][1].numpy() * rng.uniform(-1, 1, size=n)).astype(np.float32))
    v0 = torch.from_numpy((c['g'][1].numpy() ** 2 * rng.uniform(0.1, 1, size=n)).astype(np.float32))
    for betas in ((0.9, 0.999), (0.5, 0.9)):
        ref, fig, bounds = _adam_bounds(c, betas, wd, 0.125, 1, first_step=step, m0=m0, v0=v0)
        p, m, v = c['p'].to(dev), m0.to(dev), v0.to(dev)
        ops.adam_step(p, c['g'][0].to(dev), m, v, LR_ADAM, betas, EPS_ADAM, wd, 0.125, step)
        _check_adam('single step %d wd=%g betas=%s' % (step, wd, betas), p, m, v, ref, fig, bounds)


@pytest.mark.parametrize('wd', [0.0, 1e-2])
def test_flat_adam_step_against_float64(wd):
    """FlatAdam.step: one parameter of 100 003 elements over 200 steps against the same reference and bounds as ops.adam_step."""
    dev = _dev()
    from deepgate.optim import FlatAdam
    n, betas = 100003, (0.9, 0.999)
    c = _build_adam(n, K_STEPS, seed=n % 977 + 1)
    ref, fig, bounds = _adam_bounds(c, betas, wd, 1.0, K_STEPS)
    q = torch.nn.Parameter(c['p'].to(dev))
    opt = FlatAdam([q], lr=LR_ADAM, betas=betas, eps=EPS_ADAM, weight_decay=wd)
    g = c['g'].to(dev)
    for k in range(K_STEPS):
        opt.zero_grad()
        q.grad = g[k].clone()
        opt.step()
    f = opt.flat_buffers()
    _check_adam('FlatAdam n=%d wd=%g' % (n, wd), q.detach(), f['m'][:n], f['v'][:n], ref, fig, bounds)


# |p_device - p_float64| after 20 steps of at most ~lr each, |p| <= 1.02, derived: per step the stored p rounds once (2^-24 |p|), the
# step's own arithmetic is good to 8 roundings (lr * 8 * 2^-24), and 1 - beta2 = 1 - float32(0.999) differs from 0.001 by 1.3e-5
# relative, which moves v-hat, hence the step, by at most that (lr * 1.3e-5): 1.5e-6 in all.
FLAT_TOL = 20 * (U24 * 1.02 + LR_ADAM * (8 * U24 + 1.3e-5))


@pytest.mark.parametrize('wd', [0.0, 1e-2])
def test_flat_adam_odd_sizes_padding_and_a_parameter_without_gradient(wd):
    """Parameters of 1, 3, 5 and 70 elements (every view is padded to four floats) plus one whose gradient stays None, 20 steps,
    against torch.optim.Adam in float64 on the same parameters.  The padding stays zero in the parameter and both moment buffers.
    The parameter without a gradient: with weight_decay = 0 it does not move.  With weight_decay != 0 torch.optim.Adam skips it,
    while the flat kernel sees a zero gradient and DECAYS it (g = wd * p enters the moments): a documented deviation (DESIGN section 7;
    the reference's trainer uses weight_decay = 0) — pinned here as "moves exactly as Adam with a zero gradient would"."""
    dev = _dev()
    from deepgate.optim import FlatAdam
    sizes = [1, 3, 5, 70, 6]
    rng = np.random.Generator(np.random.PCG64(42))
    init = [torch.from_numpy(rng.uniform(-1, 1, size=k).astype(np.float32)) for k in sizes]
    grads = [[torch.from_numpy((rng.standard_normal(k) * 10.0 ** rng.uniform(-4, 0)).astype(np.float32)) for k in sizes] for _ in range(20)]
    params = [torch.nn.Parameter(x.to(dev)) for x in init]
    opt = FlatAdam(params, lr=LR_ADAM, betas=(0.9, 0.999), eps=EPS_ADAM, weight_decay=wd)
    tp = [torch.nn.Parameter(x.to(F64)) for x in init]
    topt = torch.optim.Adam(tp, lr=LR_ADAM, betas=(0.9, 0.999), eps=EPS_ADAM, weight_decay=wd)
    for step in range(20):
        opt.zero_grad()
        topt.zero_grad()
        for i in range(4):                                   # the fifth parameter never gets a gradient
            params[i].grad = grads[step][i].to(dev)
            tp[i].grad = grads[step][i].to(F64)
        opt.step()
        topt.step()
    for i in range(4):
        err = float((params[i].detach().cpu().to(F64) - tp[i].detach()).abs().max())
        assert err <= FLAT_TOL, (i, err)
    none_ref = LR.adam(init[4], torch.zeros(20, 6), torch.zeros(6), torch.zeros(6), LR.f32(LR_ADAM), (LR.f32(0.9), LR.f32(0.999)), LR.f32(EPS_ADAM),
                       LR.f32(wd), 1.0)
    got = params[4].detach().cpu()
    if wd == 0:
        assert torch.equal(got, init[4]) and torch.equal(tp[4].detach().float(), init[4])
    else:
        assert torch.equal(tp[4].detach().float(), init[4])                        # torch skips it
        assert float((got - init[4]).abs().min()) > 10 * LR_ADAM                   # the flat kernel decays it: ~lr per step
        assert float((got.to(F64) - none_ref['p']).abs().max()) <= FLAT_TOL
    f = opt.flat_buffers()
    pad = torch.ones(f['n'], dtype=torch.bool)
    for off, k in zip(f['offsets'], sizes):
        pad[off:off + k] = False
    assert int(pad.sum()) == 3 + 1 + 3 + 2 + 2
    for key in ('param', 'm', 'v', 'grad'):
        assert not bool(f[key].cpu()[pad].any()), key
