"""The levelised functional sweep (csrc/func_level.hip: exact fp32, H = 16 / 32 / 64; csrc/func_level_x3.hip: bf16x3, H = 32 / 64, with
span rows and packed rows, followed by mgv_sweep_pull_heavy as deepgate.ops does) and the stand-alone attention pooling
(csrc/attn_pool.hip), every entry point on its own against the float64 restatement of tests/sweep_ref.py.  That restatement is
pinned on the CPU by tests/test_sweep_spec.py, which also asserts the properties of the case builders used here and shows that the
defects these tests are there to catch are at least ten times outside their bound.

Through the C ABI: every graph table comes from a GraphPlan built on the device; buffer sizes are exactly the header's (alpha, dsc:
max(E, 1); dzb [N][2H]; scratch and heavy_ws as ops._sweep_bwd_prep sizes them; partial_ws S * H), each with 64 NaN guard rows (or
floats) behind it that must come back bit-identical.  hf is NaN-filled in front of mgv_sweep_zero_inactive + the bf16x3 forward (in
rounds >= 2: h_prev with the updated rows NaN); ghs is NaN-filled for bf16x3, which writes it, and pre-filled with a0 for fp32,
which adds to it; scratch, heavy_ws, partial_ws, dzb, alpha and dsc are NaN-filled; d_attn_u, dWvc, dbvc, dbih, dbhh are pre-filled
with a0 = S * N(0, 1) (N(0, 1) where S = 0: such an entry must come back exactly); d_gh and g_hprev are zero-filled as the header
requires, and the rows of never-updated nodes must come back exactly zero (their S is 0).

Bound: err <= tau S entry by entry, tau = 8 max(r, floor), r the worst ratio FOR THAT OUTPUT of the CPU restatement in the kernel's
arithmetic (float32, or the bf16x3 emulation) against float64 on the same case, floor = 2^-23 (fp32) or 2^-17 (bf16x3).  The fp32
backward's accumulators and the pool's du end in float atomics, one per workgroup in arrival order: their bound is max(tau, L 2^-24)
with L the chain length of the design (sweep_ref.chain_length; shown on a float32 CPU model in tests/test_sweep_spec.py).  The fp32
backward's ghs and the pool's dx have one bound per row / entry: max(tau, the float32 error of the softmax weights themselves (and,
for ghs, of dsc = alpha (t - ci)) pushed through the entry's terms), sweep_ref.alpha_error: exp turns the absolute error of a score
into a relative one of the weight, so the rows made of the spread rows' e^-60 weights alone are good to some 1e-5 in ANY float32
implementation, and which way the roundings fall there is not something the float32 restatement shares with the kernel (its r on
that row differs from one CPU to the next).  An accumulator entry additionally gets 2^-24 |a0|.  Every check prints
`SW <implementation> H=.. <case> | <output> worst err/S / largest tau, worst err/(tau S) | ...`; the last figure is the one asserted
to be at most 1.  The worst shares are in NOTEBOOK.md (2026-10-18)."""
import ctypes
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep_ref as W  # noqa: E402

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
U24 = 2.0 ** -24
GUARD = 64
NAN = float('nan')
EINVAL, EUNSUPPORTED = -1, -2

CASES = {
    's5': lambda H: W.shallow(H, 5),
    's6r': lambda H: W.shallow(H, 6, 1, rounds2=True),
    's2r': lambda H: W.shallow(H, 2, 0, rounds2=True),
    's1': lambda H: W.shallow(H, 1),
    's7': lambda H: W.shallow(H, 7),
    'n1': lambda H: W.shallow(H, 1, 4, fanout=False),          # widest level: 1, 3, 4, 5 tiles
    'n3': lambda H: W.shallow(H, 1, 0, fanout=False),
    'n4': lambda H: W.shallow(H, 5, 1, fanout=False),
    'n5': lambda H: W.shallow(H, 6, 1, fanout=False),
    'n5r': lambda H: W.shallow(H, 6, 1, rounds2=True, fanout=False),
    'deep': lambda H: W.deep(H),
    'deepr': lambda H: W.deep(H, True),
    'wide': lambda H: W.wide(H),
    'coh': lambda H: W.coherent(H),
}
ABI_CASES = ('s5', 's6r', 's2r', 's1', 'n1', 'n3', 'n4', 'n5', 'n5r', 'deep', 'deepr', 'coh')


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


@pytest.fixture(autouse=True)
def _nothing_more_after_a_gpu_error():
    """A kernel fault surfaces at the next synchronisation: the session ends there instead of launching the remaining tests on a device
    that has just reported an error."""
    yield
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit('the GPU reported an error (%s): nothing more is started on it' % e, returncode=3)


@functools.lru_cache(maxsize=None)      # one float64 run per (case, width), shared by every implementation and test that uses it
def _case(name, H):
    c = CASES[name](H)
    return c, W.sweep(c)


@functools.lru_cache(maxsize=None)
def _tau(mm, name, H):
    c, r64 = _case(name, H)
    return W.device_taus(c, r64, W.sweep(c, F32, 'x3' if mm == 'x3' else 'exact'), mm)


def _guarded(n, width, dev, fill=NAN):
    t = torch.full((n + GUARD, width) if width else (n + GUARD,), NAN, dtype=F32, device=dev)
    if fill == fill:
        t[:n] = fill
    return t


def _guard_ok(t, n):
    return bool(torch.isnan(t[n:]).all()) and bool((t[n:].view(torch.int32) == t[n:].view(torch.int32).reshape(-1)[0]).all())


def _i32(values):
    return (ctypes.c_int32 * len(values))(*values)


def _a0(S, shape, gen):
    """a0 = S * N(0, 1), N(0, 1) where S = 0; S per entry or per row."""
    u = torch.randn(*shape, generator=gen, dtype=F64)
    s = S if S.dim() == len(shape) else S[:, None]
    return torch.where(s > 0, s * u, u).to(F32)


def _scratch_elems(plan, T, H):
    """include/mgvae_hip.h: n_active * 5H + (tiles of the widest level) * T * 11H + 256 * 6H^2."""
    ltp = plan.level_tile_ptr
    widest = max([ltp[i + 1] - ltp[i] for i in range(1, len(ltp) - 1)] + [0])
    return plan.n_active * 5 * H + widest * T * 11 * H + W.WGRAD_GRID * 6 * H * H


def _sweep_abi(impl, c, r64, dev, rows=4, ws_fill=NAN, seed=1, backward=True):
    """One forward and one backward of the sweep through the C ABI.  impl 'f32' or 'x3'; rows: ints per order row (4 spans, 32 packed).
    Returns ({output: tensor}, {accumulator: a0})."""
    from deepgate import _hip, ops
    p = _hip.ptr
    H, N, T = c['H'], c['N'], c['T']
    plan = W.plan_of(c, dev)
    E = plan.E
    d = {k: c[k].to(dev) for k in ('hs', 'attn_u', 'Wvc', 'bvc', 'bih', 'bhh', 'ghf')}
    r2 = c['h_prev'] is not None
    hp = c['h_prev'].to(dev) if r2 else None
    gh = c['gh'].to(dev) if r2 else None
    upd = plan.gslot != W.NO_GATE
    ltp = _i32(plan.level_tile_ptr)
    tiles = (p(plan.tile_start), p(plan.tile_count), p(plan.tile_slot))
    hf = _guarded(N, H, dev)
    if r2:
        hf[:N] = hp
        hf[:N][upd] = NAN                                  # every updated row must be rewritten
    x3 = impl == 'x3'
    if x3:
        wpack = ops.sweep_wpack(d['Wvc'])
        rowp = (p(plan.order_rows), 32) if rows == 32 else (p(plan.order_span), 4)
        if not r2:
            _hip.call('mgv_sweep_zero_inactive', H, N, p(plan.gslot), p(hf))
        _hip.call('mgv_func_sweep_fwd_x3', H, N, T, plan.num_levels, ltp, p(plan.order), *rowp, *tiles, p(plan.in_ptr), p(plan.in_src), p(d['hs']), p(hf),
                  p(d['attn_u']), p(wpack), p(d['bvc']), p(d['bih']), p(d['bhh']), p(gh), p(hp))
    else:
        if not r2:
            hf[:N] = 0                                     # the fp32 entry: "hf must be zero on entry"
        _hip.call('mgv_func_sweep_fwd', H, N, T, plan.num_levels, ltp, p(plan.order), *tiles, p(plan.in_ptr), p(plan.in_src), p(d['hs']), p(hf),
                  p(d['attn_u']), p(d['Wvc']), p(d['bvc']), p(d['bih']), p(d['bhh']), p(gh), p(hp))
    torch.cuda.synchronize()
    assert _guard_ok(hf, N), 'forward wrote behind row N of hf'
    never = hf[:N][~upd]
    assert torch.equal(never, hp[~upd] if r2 else torch.zeros_like(never)), 'a never-updated row of hf is not its previous state'
    out = {'hf': hf[:N]}
    if not backward:
        return out, {}
    gen = torch.Generator().manual_seed(seed)
    S = r64['S']
    a0 = {k: _a0(S[k], tuple(r64[k].shape), gen) for k in W.ACCS if k in S}
    if not x3:
        a0['ghs'] = _a0(S['ghs'], (N, H), gen)
    if r2:
        a0['dbhh'] = torch.randn(T, 3 * H, generator=gen)           # (not compared in rounds >= 2; still a valid accumulator)
    acc = {}
    for k, v in a0.items():
        acc[k] = _guarded(v.shape[0], v[0].numel(), dev).reshape(v.shape[0] + GUARD, *v.shape[1:])
        acc[k][:v.shape[0]] = v.to(dev)
    ghs = acc['ghs'] if not x3 else _guarded(N, H, dev)
    dzb, alpha, dsc = _guarded(N, 2 * H, dev), _guarded(max(E, 1), 0, dev), _guarded(max(E, 1), 0, dev)
    d_gh = _guarded(N, 3 * H, dev, 0.0) if r2 else None
    g_hprev = _guarded(N, H, dev, 0.0) if r2 else None
    rnd = (p(gh), p(hp), p(d_gh), p(g_hprev))
    csr = (p(plan.in_ptr), p(plan.in_src), p(plan.out_ptr), p(plan.out_dst), p(plan.out_slot), p(plan.gslot))
    accp = [p(acc[k]) for k in W.ACCS]
    ws = []
    if x3:
        n_s = _scratch_elems(plan, T, H)
        assert ops._sweep_bwd_prep(plan, T, H, dev)[0].numel() == n_s, 'ops sizes the scratch as the header states'
        scratch = _guarded(n_s, 0, dev, ws_fill)
        ws.append((scratch, n_s, 'scratch'))
        hv = plan.heavy_segments(True, inactive_only=True)
        hav = plan.heavy_segments(True, active_by_level=True)
        if hav is None:
            ha = (0, None, None, None, None, None, None, None, 0)
        else:
            n_h = (hav['K'] + hav['S']) * 2 * H
            hws = _guarded(n_h, 0, dev, ws_fill)
            ws.append((hws, n_h, 'heavy_ws'))
            ha = (hav['K'], p(hav['nodes']), p(hav['node_seg_ptr']), p(hav['seg_e0']), p(hav['seg_e1']), _i32(hav['lvl_k_ptr']), _i32(hav['lvl_seg_ptr']),
                  p(hws), plan.HEAVY_ROW)
        _hip.call('mgv_func_sweep_bwd_x3', H, N, T, plan.num_levels, ltp, p(plan.order), *rowp, plan.n_active, *tiles, p(plan.slot_tiles),
                  _i32(plan.slot_tile_ptr), *csr, p(d['hs']), p(hf), p(d['attn_u']), p(wpack), p(d['bvc']), p(d['bih']), p(d['bhh']), p(d['ghf']), p(ghs),
                  p(dzb), p(alpha), p(dsc), *accp, p(scratch), n_s, plan.HEAVY_ROW if hv is not None else 0, *ha, *rnd)
        if hv is not None:
            pw = _guarded(hv['S'] * H, 0, dev, ws_fill)
            ws.append((pw, hv['S'] * H, 'partial_ws'))
            _hip.call('mgv_sweep_pull_heavy', H, hv['K'], p(hv['nodes']), p(hv['node_seg_ptr']), hv['S'], p(hv['seg_e0']), p(hv['seg_e1']), p(plan.out_dst),
                      p(plan.out_slot), p(plan.gslot), p(alpha), p(dsc), p(dzb), p(d['attn_u']), p(pw), p(ghs))
    else:
        WvcT = d['Wvc'].transpose(1, 2).contiguous()
        _hip.call('mgv_func_sweep_bwd', H, N, T, plan.num_levels, ltp, p(plan.order), *tiles, *csr, p(d['hs']), p(hf), p(d['attn_u']), p(d['Wvc']), p(WvcT),
                  p(d['bvc']), p(d['bih']), p(d['bhh']), p(d['ghf']), p(ghs), p(dzb), p(alpha), p(dsc), *accp, *rnd)
    torch.cuda.synchronize()
    for t, n, what in ws:
        assert bool(torch.isnan(t[n:]).all()), 'the backward wrote behind ' + what
    for t, n, what in ((ghs, N, 'ghs'), (dzb, N, 'dzb'), (alpha, max(E, 1), 'alpha'), (dsc, max(E, 1), 'dsc')) + tuple((acc[k], a0[k].shape[0], k) for k in W.ACCS):
        assert _guard_ok(t, n), 'the backward wrote behind ' + what
    out['ghs'] = ghs[:N]
    for k in W.ACCS:
        out[k] = acc[k][:a0[k].shape[0]]
    if r2:
        assert _guard_ok(d_gh, N) and _guard_ok(g_hprev, N), 'the backward wrote behind d_gh / g_hprev'
        out['d_gh'], out['g_hprev'] = d_gh[:N], g_hprev[:N]
        a0.pop('dbhh')
        out.pop('dbhh')
    # what nobody writes stays as it was: the per-edge scratch of never-updated consumers
    dst_never = ~upd[plan.in_dst.long()] if E else torch.zeros(0, dtype=torch.bool, device=dev)
    assert bool(torch.isnan(alpha[:E][dst_never]).all()) and bool(torch.isnan(dzb[:N][~upd]).all()), 'scratch of a never-updated consumer was written'
    assert bool(torch.isfinite(alpha[:E][~dst_never]).all()) and bool(torch.isfinite(dsc[:E][~dst_never]).all()) and bool(torch.isfinite(dzb[:N][upd]).all())
    out['_edge'] = (alpha[:E], dsc[:E], dzb[:N])
    return out, a0


def _compare(tag, got, a0, r64, tau, collect=None):
    """err <= tau S entry by entry (module docstring; tau[k] a float, or one value per entry of S[k]).  Prints per output the worst
    err / S over the largest tau and, behind it, the worst err / (tau S), which is what is asserted to be at most 1."""
    line, bad = [], []
    for k, v in got.items():
        if k.startswith('_') or k not in r64['S']:
            continue
        v = v.detach().cpu().to(F64)
        ref, S, t = r64[k], r64['S'][k], tau[k]
        if k in a0:
            b = a0[k].to(F64)
            wide = (lambda s: s if s.dim() == b.dim() else s[:, None].expand_as(b))      # noqa: E731
            Sb = wide(S)
            tb = wide(t) if torch.is_tensor(t) else t
            zero = Sb == 0
            if bool(zero.any()) and not torch.equal(v[zero].to(F32), a0[k][zero]):
                bad.append('%s: an entry nothing contributes to changed' % k)
            err = (((v - b) - ref).abs() - U24 * b.abs()).clamp(min=0)
            q = (err / Sb.clamp(min=1e-300))[~zero]
            qt = (err / (Sb * tb).clamp(min=1e-300))[~zero]
            r, sh = (float(q.max()), float(qt.max())) if q.numel() else (0.0, 0.0)
            if not bool(torch.isfinite(v).all()):
                r = sh = float('inf')
        else:
            r, sh = W.ratio(v, ref, S), W.share(v, ref, S, t)
        line.append('%s %.2g/%.2g %.2f' % (k, r, W.tau_max(t), sh))
        if collect is not None:
            collect[k] = max(collect.get(k, 0.0), sh)
        if not sh <= 1:
            bad.append('%s: %.3g of its scale, %.3g of its bound (largest bound %.3g)' % (k, r, sh, W.tau_max(t)))
    print('SW %s | %s' % (tag, ' | '.join(line)))
    return bad


def _check(impl, name, H, rows=4, **opts):
    c, r64 = _case(name, H)
    got, a0 = _sweep_abi(impl, c, r64, _dev(), rows=rows, **opts)
    return ['%s: %s' % (name, b) for b in _compare('%s H=%d rows=%d %s' % (impl, H, rows, c['name']), got, a0, r64, _tau(impl, name, H))]


# ------------------------------------------------------------------------------------------------ the sweep through the C ABI
@pytest.mark.parametrize('name', ABI_CASES)
@pytest.mark.parametrize('H', [16, 32, 64])
def test_fp32_sweep_against_float64(H, name):
    """mgv_func_sweep_fwd / _bwd on the shallow cases (every fan-in, fan-out, slot absence, spread and equal rows, never-updated
    sources and consumers, T in {1, 2, 5, 6}, rounds 1 and >= 2), the deep ones and the coherent one."""
    bad = _check('f32', name, H)
    assert not bad, bad


@pytest.mark.parametrize('name', ABI_CASES)
@pytest.mark.parametrize('rows', [4, 32])
@pytest.mark.parametrize('H', [32, 64])
def test_x3_sweep_against_float64(H, rows, name):
    """mgv_sweep_zero_inactive + mgv_func_sweep_fwd_x3, mgv_func_sweep_bwd_x3 + mgv_sweep_pull_heavy on the same cases, with span rows
    (4 ints) and packed rows (32 ints).  The shallow cases reach kInRegs = 3 / kInCap = 4 (fan-in 3, 4, 5), kOutChunk = 2, kRowOut = 8,
    kOutCap = 16 (fan-out 2, 3, 8, 9, 16, 17), HEAVY_ROW = 64 and HEAVY_SEG = 512 (64, 65, 513, 1100 consumers on an input and on a
    level-1 gate: both pre-passes, 1, 2 and 3 segments) and 1, 3, 4, 5 tiles in the widest level."""
    bad = _check('x3', name, H, rows)
    assert not bad, bad


@pytest.mark.parametrize('impl,H', [('f32', 32), ('f32', 64), ('x3', 32), ('x3', 64)])
def test_wide_level_against_float64(impl, H):
    """257 tiles of one slot in one level (kWgradGrid = 256: workgroup 0 of the weight-gradient kernel takes a second tile) and N one
    past the grid cap of the inactive pull (sweep_ref.GEOMETRY)."""
    bad = _check(impl, 'wide', H)
    assert not bad, bad


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('impl,H', [('f32', 16), ('f32', 64), ('x3', 32), ('x3', 64)])
def test_forward_is_deterministic(impl, H):
    dev = _dev()
    for name in ('s5', 's6r'):
        c, r64 = _case(name, H)
        a, _ = _sweep_abi(impl, c, r64, dev, backward=False)
        b, _ = _sweep_abi(impl, c, r64, dev, backward=False)
        assert torch.equal(_bits(a['hf']), _bits(b['hf'])), name


@pytest.mark.parametrize('rows', [4, 32])
def test_x3_backward_is_deterministic_and_ignores_what_lies_in_its_workspaces(rows):
    """include/mgvae_hip.h and DESIGN.md 4.4: no float atomics at H = 64.  Twice, with NaN and then 1e30 in scratch, heavy_ws and
    partial_ws: the same bits in every output and in the per-edge scratch."""
    dev = _dev()
    for name in ('s5', 's6r'):
        c, r64 = _case(name, 64)
        a, _ = _sweep_abi('x3', c, r64, dev, rows=rows)
        b, _ = _sweep_abi('x3', c, r64, dev, rows=rows, ws_fill=1e30)
        for k in a:
            if k == '_edge':
                continue
            assert torch.equal(_bits(a[k]), _bits(b[k])), (name, k)
        upd = W.plan_of(c, dev).gslot != W.NO_GATE
        assert torch.equal(_bits(a['_edge'][2][upd]), _bits(b['_edge'][2][upd])), (name, 'dzb')


@pytest.mark.parametrize('H', [32, 64])
def test_heavy_pull_alone_against_float64(H):
    """mgv_sweep_pull_heavy on the float64 run's own alpha, dsc and dzb (rounded to float32): the ghs rows of the heavy never-updated
    nodes (65, 513, 1100 consumers: 1, 2 and 3 segments), every other row untouched."""
    from deepgate import _hip
    p = _hip.ptr
    dev = _dev()
    c, r64 = _case('s5', H)
    plan = W.plan_of(c, dev)
    hv = plan.heavy_segments(True, inactive_only=True)
    N, E = c['N'], plan.E
    alpha, dsc, dzb = (r64[k].to(F32).to(dev) for k in ('alpha', 'dsc', 'dzb'))
    never = plan.gslot != W.NO_GATE
    dzb[~never] = NAN                                       # nobody wrote them in the product either
    ghs = _guarded(N, H, dev)
    pw = _guarded(hv['S'] * H, 0, dev)
    _hip.call('mgv_sweep_pull_heavy', H, hv['K'], p(hv['nodes']), p(hv['node_seg_ptr']), hv['S'], p(hv['seg_e0']), p(hv['seg_e1']), p(plan.out_dst),
              p(plan.out_slot), p(plan.gslot), p(alpha), p(dsc), p(dzb), p(c['attn_u'].to(dev)), p(pw), p(ghs))
    torch.cuda.synchronize()
    nodes = hv['nodes'].long()
    assert {65, 513, 1100} <= set(int(plan.out_ptr[v + 1] - plan.out_ptr[v]) for v in nodes.tolist())
    assert bool(torch.isnan(pw[hv['S'] * H:]).all()) and _guard_ok(ghs, N)
    rest = torch.ones(N, dtype=torch.bool, device=dev)
    rest[nodes] = False
    assert bool(torch.isnan(ghs[:N][rest]).all()), 'a row outside the list was written'
    nc = nodes.cpu()
    r = W.ratio(ghs[:N][nodes], r64['ghs'][nc], r64['S']['ghs'][nc])
    # the float32 CPU model of the same sum: the same float32 terms added in list order
    cp = W.plan_of(c)
    live = torch.nonzero(cp.gslot[cp.in_dst.long()] != W.NO_GATE).reshape(-1)
    dl = cp.in_dst.long()[live]
    term = alpha.cpu()[live, None] * r64['dzb'].to(F32)[dl, :H] + dsc.cpu()[live, None] * c['attn_u'][cp.gslot[dl].long(), :H]
    model = torch.zeros(N, H).index_add_(0, cp.in_src.long()[live], term)
    tau = 8 * max(W.ratio(model[nc], r64['ghs'][nc], r64['S']['ghs'][nc]), W.FLOOR['f32'])
    print('SW pull_heavy H=%d ghs %.2g/%.2g' % (H, r, tau))
    assert r <= tau, (r, tau)


# ------------------------------------------------------------------------------------------------ through deepgate.ops
def _through_ops(name, H, mm):
    from deepgate import ops
    dev = _dev()
    c, r64 = _case(name, H)
    plan = W.plan_of(c, dev)
    plan.cache.drop('order_rows', 'sweep_steps')
    leaf = lambda t: t.to(dev).clone().requires_grad_(True)       # noqa: E731
    hs, u, Wvc, bvc, bih = (leaf(c[k]) for k in ('hs', 'attn_u', 'Wvc', 'bvc', 'bih'))
    r2 = c['h_prev'] is not None
    bhh = None if r2 else leaf(c['bhh'])
    hp, gh = (leaf(c['h_prev']), leaf(c['gh'])) if r2 else (None, None)
    hf = ops.FuncSweepFn.apply(plan, hs, u, Wvc, bvc, bih, bhh, hp, gh)
    hf.backward(c['ghf'].to(dev))
    got = {'hf': hf.detach(), 'ghs': hs.grad, 'd_attn_u': u.grad, 'dWvc': Wvc.grad, 'dbvc': bvc.grad, 'dbih': bih.grad}
    if r2:
        got['d_gh'], got['g_hprev'] = gh.grad, hp.grad
    else:
        got['dbhh'] = bhh.grad
    return _compare('ops %s H=%d %s' % (mm, H, c['name']), got, {}, r64, _tau(mm, name, H))


@pytest.mark.parametrize('packed', [0, 2])
@pytest.mark.parametrize('H', [32, 64])
def test_through_ops_bf16x3(H, packed, monkeypatch):
    from deepgate import ops
    monkeypatch.setattr(ops, 'PACKED_ROWS', packed)
    monkeypatch.setattr(ops, 'PRECISION', 'x3')
    monkeypatch.delenv('MGV_SWEEP_X3', raising=False)
    bad = []
    for name in ('s5', 's6r', 'deepr', 'n5'):
        bad += _through_ops(name, H, 'x3')
    assert not bad, bad


@pytest.mark.parametrize('H', [16, 32, 64])
def test_through_ops_fp32_and_seven_slots(H, monkeypatch):
    """MGV_SWEEP_X3=0 sends every width to the fp32 kernels; T = 7 is above kMaxSlots = 6 and goes there on its own (the bf16x3 entry
    refuses it: test_refusals)."""
    from deepgate import ops
    monkeypatch.setattr(ops, 'PRECISION', 'x3')
    monkeypatch.delenv('MGV_SWEEP_X3', raising=False)
    assert not ops._sweep_x3(H, 7) and ops._sweep_x3(H, 6) == (H in (32, 64))
    bad = _through_ops('s7', H, 'f32')
    monkeypatch.setenv('MGV_SWEEP_X3', '0')
    for name in ('s5', 's6r'):
        bad += _through_ops(name, H, 'f32')
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ attention pooling
@functools.lru_cache(maxsize=None)
def _pool(Wd, N):
    c = W.pool_case(Wd, N)
    r64 = W.attn_pool(c)
    tau = {k: 8 * max(v, W.FLOOR['f32']) for k, v in W.ratios(W.attn_pool(c, F32), r64).items()}
    # du ends in float atomics: a lane group adds its nodes' edges one after another, the groups of a workgroup are summed in LDS and
    # every workgroup adds its share with one atomic, in arrival order: L = longest chain of one group + groups + workgroups
    # (measured on an MI355X at N = 16,385: 6.5e-6 of scale against tau = 9.5e-7; L 2^-24 = 1.3e-4 there)
    groups = W.THREADS // (Wd // 4)
    grid = W.grid_for((N + groups - 1) // groups, 8)
    deg = (c['ptr'][1:] - c['ptr'][:-1])
    L = int(deg.max()) + 3 * ((N + grid * groups - 1) // (grid * groups)) + groups + grid
    tau['du'] = max(tau['du'], L * U24)
    # dx of the spread rows' middle source is two weights e^-60 times dz and nothing else: one bound per entry, max(tau, alpha's own
    # float32 error pushed through the entry's terms) (sweep_ref.alpha_error), as for the fp32 sweep's ghs
    tau['dx'] = r64['aux']['dx_alpha'].clamp(min=tau['dx'])
    return c, r64, tau


def _pool_sizes(Wd):
    return (1, 2, 20, W.cap_rows('attn_pool', Wd) + 1)


@pytest.mark.parametrize('Wd', [32, 64, 128])
def test_attn_pool_against_float64(Wd):
    """mgv_attn_pool_fwd / _bwd: lists of 0, 1, 2, 3, 64, 65 and 3000 entries, a repeated source, the spread rows, N = 1, 2, 20 and
    one past the grid cap; zbar, mstat, inv behind guard rows, dx and du pre-filled with a0."""
    from deepgate import _hip
    p = _hip.ptr
    dev = _dev()
    bad = []
    for N in _pool_sizes(Wd):
        c, r64, tau = _pool(Wd, N)
        d = {k: c[k].to(dev) for k in ('x', 'u', 'dz', 'ptr', 'idx')}
        zbar, m, inv = _guarded(N, Wd, dev), _guarded(N, 0, dev), _guarded(N, 0, dev)
        _hip.call('mgv_attn_pool_fwd', Wd, N, p(d['ptr']), p(d['idx']), p(d['x']), p(d['u']), p(zbar), p(m), p(inv))
        torch.cuda.synchronize()
        assert _guard_ok(zbar, N) and _guard_ok(m, N) and _guard_ok(inv, N), 'the forward wrote behind row N'
        z2, m2, i2 = _guarded(N, Wd, dev), _guarded(N, 0, dev), _guarded(N, 0, dev)
        _hip.call('mgv_attn_pool_fwd', Wd, N, p(d['ptr']), p(d['idx']), p(d['x']), p(d['u']), p(z2), p(m2), p(i2))
        assert torch.equal(_bits(zbar[:N]), _bits(z2[:N])) and torch.equal(_bits(m[:N]), _bits(m2[:N])) and torch.equal(_bits(inv[:N]), _bits(i2[:N]))
        gen = torch.Generator().manual_seed(2)
        a0 = {'dx': _a0(r64['S']['dx'], (c['R'], Wd), gen), 'du': _a0(r64['S']['du'], (Wd,), gen)}
        dx, du = _guarded(c['R'], Wd, dev), _guarded(Wd, 0, dev)
        dx[:c['R']], du[:Wd] = a0['dx'].to(dev), a0['du'].to(dev)
        _hip.call('mgv_attn_pool_bwd', Wd, N, p(d['ptr']), p(d['idx']), p(d['x']), p(d['u']), p(zbar), p(m), p(inv), p(d['dz']), p(dx), p(du))
        torch.cuda.synchronize()
        assert _guard_ok(dx, c['R']) and _guard_ok(du, Wd), 'the backward wrote behind its outputs'
        got = {'zbar': zbar[:N], 'mstat': m[:N], 'inv': inv[:N], 'dx': dx[:c['R']], 'du': du[:Wd]}
        bad += ['N=%d %s' % (N, b) for b in _compare('pool W=%d N=%d' % (Wd, N), got, a0, r64, tau)]
    assert not bad, bad


@pytest.mark.parametrize('Wd', [32, 128])
def test_attn_pool_through_ops(Wd):
    from deepgate import ops
    from deepgate.graph_plan import GraphPlan
    dev = _dev()
    c, r64, tau = _pool(Wd, 20)
    ptr = c['ptr'].long()
    dst = torch.repeat_interleave(torch.arange(c['N']), ptr[1:] - ptr[:-1])
    plan = GraphPlan(torch.stack([c['idx'][:c['E']].long(), dst]).to(dev), c['R'])
    x, u = c['x'].to(dev).requires_grad_(True), c['u'].to(dev).requires_grad_(True)
    zbar = ops.AttnPoolFn.apply(x, u, plan)
    g = torch.zeros(c['R'], Wd)
    g[:c['N']] = c['dz']
    zbar.backward(g.to(dev))
    assert float(zbar[c['N']:].abs().max()) == 0
    bad = _compare('pool ops W=%d' % Wd, {'zbar': zbar[:c['N']].detach(), 'dx': x.grad, 'du': u.grad}, {}, r64, tau)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ refusals
def _rc(name, *args):
    from deepgate import _hip
    return getattr(_hip.load(), name)(*args, _hip.stream())


def test_refusals_come_back_by_return_code_with_the_outputs_untouched():
    """T = 7 and H = 16 on the bf16x3 entries, order_span_ints = 8, gh without h_prev, scratch_elems one short, W = 48 and widths 0 .. 3
    (which used to divide by zero on the host), and an unsupported H on a sweep without a tile (all four entries agree): a return
    code, nothing launched, every output bit-identical.  Every buffer is valid and of the header's size all the same."""
    from deepgate import _hip, ops
    from deepgate.graph_plan import GraphPlan
    p = _hip.ptr
    dev = _dev()

    def attempt(c, H, T, span_ints=4, gh_only=False, short=0, entries=('fwd_x3', 'bwd_x3')):
        N = c['N']
        plan = W.plan_of(c, dev)
        E = plan.E
        d = {k: c[k].to(dev) for k in ('hs', 'attn_u', 'Wvc', 'bvc', 'bih', 'bhh', 'ghf')}
        wpack = torch.zeros(max(T, 1) * 4 * 6 * max(H, 16) ** 2, dtype=torch.bfloat16, device=dev)
        outs = {k: torch.full(s, NAN, dtype=F32, device=dev) for k, s in
                (('hf', (N, c['H'])), ('ghs', (N, c['H'])), ('dzb', (N, 2 * c['H'])), ('alpha', (max(E, 1),)), ('dsc', (max(E, 1),)), ('d_attn_u', (T, 2 * c['H'])),
                 ('dWvc', (T, 3 * c['H'], 2 * c['H'])), ('dbvc', (T, 3 * c['H'])), ('dbih', (T, 3 * c['H'])), ('dbhh', (T, 3 * c['H'])))}
        n_s = _scratch_elems(plan, T, c['H'])
        scratch = torch.full((n_s,), NAN, dtype=F32, device=dev)
        hav = plan.heavy_segments(True, active_by_level=True)
        if hav is None:
            ha = (0, None, None, None, None, None, None, None, 0)
        else:
            hws = torch.full(((hav['K'] + hav['S']) * 2 * c['H'],), NAN, dtype=F32, device=dev)
            ha = (hav['K'], p(hav['nodes']), p(hav['node_seg_ptr']), p(hav['seg_e0']), p(hav['seg_e1']), _i32(hav['lvl_k_ptr']), _i32(hav['lvl_seg_ptr']),
                  p(hws), plan.HEAVY_ROW)
        gh = torch.zeros(N, 3 * c['H'], device=dev) if gh_only else None
        ltp = _i32(plan.level_tile_ptr)
        tiles = (p(plan.tile_start), p(plan.tile_count), p(plan.tile_slot))
        csr = (p(plan.in_ptr), p(plan.in_src), p(plan.out_ptr), p(plan.out_dst), p(plan.out_slot), p(plan.gslot))
        par = (p(d['bvc']), p(d['bih']), p(d['bhh']))
        accp = [p(outs[k]) for k in W.ACCS]
        rcs = {}
        if 'fwd_x3' in entries:
            rcs['fwd_x3'] = _rc('mgv_func_sweep_fwd_x3', H, N, T, plan.num_levels, ltp, p(plan.order), p(plan.order_span), span_ints, *tiles, p(plan.in_ptr),
                                p(plan.in_src), p(d['hs']), p(outs['hf']), p(d['attn_u']), p(wpack), *par, p(gh), None)
        if 'bwd_x3' in entries:
            rcs['bwd_x3'] = _rc('mgv_func_sweep_bwd_x3', H, N, T, plan.num_levels, ltp, p(plan.order), p(plan.order_span), span_ints, plan.n_active, *tiles,
                                p(plan.slot_tiles), _i32(plan.slot_tile_ptr), *csr, p(d['hs']), p(d['hs']), p(d['attn_u']), p(wpack), *par, p(d['ghf']),
                                p(outs['ghs']), p(outs['dzb']), p(outs['alpha']), p(outs['dsc']), *accp, p(scratch), n_s - short, 0, *ha, p(gh), None, None, None)
        if 'fwd' in entries:
            rcs['fwd'] = _rc('mgv_func_sweep_fwd', H, N, T, plan.num_levels, ltp, p(plan.order), *tiles, p(plan.in_ptr), p(plan.in_src), p(d['hs']),
                             p(outs['hf']), p(d['attn_u']), p(d['Wvc']), *par, p(gh), None)
        if 'bwd' in entries:
            rcs['bwd'] = _rc('mgv_func_sweep_bwd', H, N, T, plan.num_levels, ltp, p(plan.order), *tiles, *csr, p(d['hs']), p(d['hs']), p(d['attn_u']),
                             p(d['Wvc']), p(d['Wvc']), *par, p(d['ghf']), p(outs['ghs']), p(outs['dzb']), p(outs['alpha']), p(outs['dsc']), *accp, p(gh), None, None, None)
        torch.cuda.synchronize()
        for k, t in list(outs.items()) + [('scratch', scratch)]:
            assert bool(torch.isnan(t).all()) and bool((_bits(t) == _bits(t).reshape(-1)[0]).all()), (k, 'touched by a refused call')
        return rcs

    c7, _ = _case('s7', 32)
    assert attempt(c7, 32, 7) == {'fwd_x3': EINVAL, 'bwd_x3': EINVAL}
    c16, _ = _case('s5', 16)                                # (with heavy lists on updated gates: nothing of their pre-pass may start)
    assert attempt(c16, 16, 5) == {'fwd_x3': EUNSUPPORTED, 'bwd_x3': EUNSUPPORTED}
    c32, _ = _case('s5', 32)
    assert attempt(c32, 32, 5, span_ints=8) == {'fwd_x3': EINVAL, 'bwd_x3': EINVAL}
    assert attempt(c32, 32, 5, gh_only=True, entries=('fwd_x3', 'bwd_x3', 'fwd', 'bwd')) == {'fwd_x3': EINVAL, 'bwd_x3': EINVAL, 'fwd': EINVAL, 'bwd': EINVAL}
    assert attempt(c32, 32, 5, short=1, entries=('bwd_x3',)) == {'bwd_x3': EINVAL}
    # a sweep without a tile (four inputs, no edge): every entry refuses a width it does not serve, 0 .. 3 included
    import numpy as np
    e = {'H': 32, 'T': 1, 'N': 4, 'gate_ids': [1], 'ei': np.zeros((2, 0), dtype=np.int64), 'gate': np.zeros(4, dtype=np.int64), 'level': np.zeros(4, dtype=np.int64),
         'hs': torch.zeros(4, 32), 'attn_u': torch.zeros(1, 64), 'Wvc': torch.zeros(1, 96, 64), 'bvc': torch.zeros(1, 96), 'bih': torch.zeros(1, 96),
         'bhh': torch.zeros(1, 96), 'ghf': torch.zeros(4, 32)}
    assert W.plan_of(e, dev).num_tiles == 0
    for H in (0, 1, 2, 3, 48, 128):
        assert attempt(e, H, 1, entries=('fwd_x3', 'bwd_x3', 'fwd', 'bwd')) == {k: EUNSUPPORTED for k in ('fwd_x3', 'bwd_x3', 'fwd', 'bwd')}, H
    assert attempt(e, 16, 1, entries=('fwd_x3', 'bwd_x3')) == {'fwd_x3': EUNSUPPORTED, 'bwd_x3': EUNSUPPORTED}
    # attention pooling
    c, _, _ = _pool(32, 20)
    d = {k: c[k].to(dev) for k in ('x', 'u', 'dz', 'ptr', 'idx')}
    outs = [torch.full(s, NAN, dtype=F32, device=dev) for s in ((20, 32), (20,), (20,), (c['R'], 32), (32,))]
    for Wd in (48, 0, 1, 2, 3, 16, 256):
        assert _rc('mgv_attn_pool_fwd', Wd, 20, p(d['ptr']), p(d['idx']), p(d['x']), p(d['u']), p(outs[0]), p(outs[1]), p(outs[2])) == EUNSUPPORTED, Wd
        assert _rc('mgv_attn_pool_bwd', Wd, 20, p(d['ptr']), p(d['idx']), p(d['x']), p(d['u']), p(d['x']), p(d['u']), p(d['u']), p(d['dz']), p(outs[3]),
                   p(outs[4])) == EUNSUPPORTED, Wd
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in outs)
    with pytest.raises(ValueError):
        ops.AttnPoolFn.apply(torch.zeros(4, 48, device=dev), torch.zeros(48, device=dev), GraphPlan(torch.zeros(2, 0, dtype=torch.long, device=dev), 4))
